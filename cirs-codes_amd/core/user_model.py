"""UserModel (reference core/user_model.py:29-581): the base class of the CIRS user models — training loop surface
(`compile`, `fit_data`), static-baseline recommendation (`compile_UCB`, `recommend_k_item`) — delegating every computation to
the device model of the subclass (`device_model()` -> cirs_hip.deepfm.DeviceDeepFM, `cirs_deepfm_train_epoch`,
`cirs_select_items`), and the validation pass (`predict_data`, `evaluate_data`: cirs_hip.userval, one launch over the resident
validation set).  Subclasses build the parameters under the reference's state_dict names (UserModel_Pairwise)."""
import numpy as np
import torch
from torch import nn

from core.inputs import compute_input_dim  # noqa: F401  (re-exported like the reference module does)
from deepctr_torch.inputs import build_input_features  # noqa: F401


def metric_mae(y, y_predict):
    """The "mae" lambda of the Kuaishou scripts (CIRS-UserModel-kuaishou.py:207): mean |y - y_predict| over float64 arrays."""
    return nn.functional.l1_loss(torch.from_numpy(np.asarray(y, np.float64)), torch.from_numpy(np.asarray(y_predict, np.float64))).numpy()


def metric_mse(y, y_predict):
    """The "mse" lambda of the Kuaishou scripts (CIRS-UserModel-kuaishou.py:209): mean (y - y_predict)^2 over float64 arrays."""
    return nn.functional.mse_loss(torch.from_numpy(np.asarray(y, np.float64)), torch.from_numpy(np.asarray(y_predict, np.float64))).numpy()


# evaluate_data recognises the two by this attribute (like `loss_kind` / `lambda_ab` mark the losses) and takes them from the sums
# the validation kernel reduces on the device, sum / n in float64, without reading the predictions back
metric_mae.device_metric = "mae"
metric_mse.device_metric = "mse"


class UserModel(nn.Module):
    seed_rec = 2022
    RL_eval_fun = None
    metric_fun = None

    def device_model(self):
        raise NotImplementedError("subclasses bind their parameters to a device model")

    # ---- training (reference core/user_model.py:74-170) ---------------------------------------------------------------
    def compile(self, optimizer, loss_dict=None, metrics=None, metric_fun=None, loss_func=None):
        assert optimizer == "adam" or isinstance(optimizer, torch.optim.Adam), "the device step implements torch.optim.Adam"
        assert loss_func is not None and (hasattr(loss_func, "lambda_ab") or hasattr(loss_func, "loss_kind")), \
            "pass core.user_model_pairwise.make_loss_kuaishou_pairwise(lambda_ab), loss_kuaishou_IPS_pairwise or " \
            "loss_kuaishou_PD_pairwise: the loss runs inside the device training step"
        assert getattr(loss_func, "loss_kind", "pairwise") == "pairwise" or self.ab_columns is None, \
            "the IPS and PD losses take no alpha/beta: build the model without ab_columns"
        self.metrics_names = ["loss"]
        self.loss_func, self.metric_fun, self.metrics = loss_func, metric_fun, metrics
        self.optim = "adam"
        self._lr = optimizer.param_groups[0]["lr"] if isinstance(optimizer, torch.optim.Adam) else 1e-3

    def compile_RL_test(self, RL_eval_fun):
        """reference core/user_model.py:71-72: fit_data evaluates fn(self.eval()) before training and after every epoch."""
        self.RL_eval_fun = RL_eval_fun

    # ---- validation (reference core/user_model.py:351-399) --------------------------------------------------------------
    def _new_trainer(self):
        from cirs_hip.deepfm_train import DeepFMTrainer
        return DeepFMTrainer(self.state_dict(), use_ab=self.ab_columns is not None, lambda_ab=getattr(self.loss_func, "lambda_ab", 0.0),
                             l2_embedding=self._l2[0], l2_linear=self._l2[1], l2_all=self._l2[2], lr=self._lr,
                             loss_kind=getattr(self.loss_func, "loss_kind", "pairwise"))

    def _valset(self, dataset):
        """The data set's x [n,7] / y resident on the device in the kernel's column form, ids checked once (kept on the data set)."""
        from cirs_hip.userval import ValSet
        dm = self.device_model()
        key = (id(dataset.x_numpy), id(dataset.y_numpy))
        cached = getattr(dataset, "_device_valset", None)
        if cached is None or cached[0] != key or cached[1].vocab != (dm.cfg.n_user_vocab, dm.cfg.n_item_vocab, dm.cfg.n_feat_vocab):
            cached = (key, ValSet(dataset.x_numpy, dataset.get_y(), dm.cfg, dm.device))
            dataset._device_valset = cached
        return cached[1]

    def predict_data(self, dataset_predict, batch_size=256, verbose=False):
        """forward over every row of the data set -> np.float64 [n,1] (core/user_model.py:361-399).  One launch of the tile kernel over
        the resident set; `batch_size` is accepted and has no effect."""
        pred, _ = self.device_model().validate(self._valset(dataset_predict), want_pred=True, want_sums=False)
        return pred.cpu().numpy().astype("float64").reshape(-1, 1)

    def _metrics_of(self, validate, valset, dataset_val):
        """{name: float} over self.metric_fun from one validate(valset, want_pred, want_sums) call: a metric tagged `device_metric`
        is sum / n of the fused float64 sums, any other callable gets (y, predictions) like the reference; with every metric tagged
        no prediction is written."""
        from cirs_hip.userval import DEVICE_METRICS
        tagged = {name: getattr(fn, "device_metric", None) in DEVICE_METRICS for name, fn in self.metric_fun.items()}
        want_pred, want_sums = not all(tagged.values()), any(tagged.values())
        pred, sums = validate(valset, want_pred=want_pred, want_sums=want_sums)
        sums = sums.cpu().numpy() if want_sums else None
        y_predict = pred.cpu().numpy().astype("float64").reshape(-1, 1) if want_pred else None
        result = {}
        for name, fn in self.metric_fun.items():
            if tagged[name]:
                result[name] = float(sums[DEVICE_METRICS.index(fn.device_metric)] / valset.n)
            else:
                result[name] = float(fn(dataset_val.get_y(), y_predict))
        return result

    def evaluate_data(self, dataset_val, batch_size=256):
        """{name: float} over the metric_fun of compile() (core/user_model.py:351-359)."""
        assert self.metric_fun, "compile(metric_fun={...}) first"
        return self._metrics_of(self.device_model().validate, self._valset(dataset_val), dataset_val)

    def _publish(self):
        """The trained parameters into the module, under its state_dict names: one device copy of the parameter buffer."""
        with torch.no_grad():
            mine = dict(self.named_parameters())
            for k, v in self._trainer.state_dict().items():
                if k in mine:
                    mine[k].copy_(v.reshape(mine[k].shape).to(mine[k].device))
        self._dev = None

    _loss_columns = (0, 4)      # {loss, reg_loss} of the trainer's per-step loss rows

    def fit_data(self, dataset_train, dataset_val=None, batch_size=256, epochs=1, verbose=1, initial_epoch=0, callbacks=None, shuffle=True):
        """One pass per epoch over (x, y, score) minibatches: the data set is made resident on the device once, every epoch is one
        train_epoch call over the permutation drawn here, and the losses are read back once per epoch.  With a validation set and a
        non-empty metric_fun, and / or compile_RL_test, the validation metrics (one launch over the resident validation set, on the
        trainer's live parameters) and the hook's results join the logs of epoch -1 (the untrained model) and of every epoch, in the
        order of core/user_model.py:123-135, 204-240.  The parameters are published into the module at the end of every epoch, in
        front of the hook and the callbacks, so both see the weights of their epoch."""
        assert self.optim is not None, "call compile() first"
        if self._trainer is None:
            self._trainer = self._new_trainer()
        tr = self._trainer
        n_all = tr.load(dataset_train.x_numpy, dataset_train.y_numpy, dataset_train.score)
        valset = self._valset(dataset_val) if dataset_val is not None and self.metric_fun else None
        callbacks = callbacks or []
        for cb in callbacks:
            cb.on_train_begin()

        def report(logs):
            if valset is not None:
                logs.update(self._metrics_of(tr.validate, valset, dataset_val))
            if self.RL_eval_fun:
                for name, result in self.RL_eval_fun(self.eval()).items():
                    logs[name] = result
            return logs

        if valset is not None or self.RL_eval_fun:      # core/user_model.py:123-135
            logs = report({})
            for cb in callbacks:
                cb.on_epoch_end(-1, logs)
        history = []
        c_loss, c_reg = self._loss_columns
        for epoch in range(initial_epoch, epochs):
            for cb in callbacks:
                cb.on_epoch_begin(epoch)
            order = torch.randperm(n_all, device=tr.device) if shuffle else None
            lo = tr.epoch(order, batch_size, check=False)
            loss_sum = float((lo[:, c_loss] + lo[:, c_reg]).double().sum())     # the fp32 step totals summed in float64, like `+= total_loss.item()`
            logs = {"loss": loss_sum / n_all}              # total_loss_epoch / sample_num (core/user_model.py:205)
            self._publish()
            report(logs)                                   # core/user_model.py:210-219
            history.append(logs)
            for cb in callbacks:
                cb.on_epoch_end(epoch, logs)
        for cb in callbacks:
            cb.on_train_end()
        self._publish()
        return history

    # ---- offline ranking evaluation against the fully observed env matrix (no reference counterpart) ----------------------
    def evaluate_ranking(self, env, dataset_val, k, *, rel_threshold=None, users=None, batch_users=1024):
        """Top-k lists of the model for env users (`users`: env numbering, default all of them) scored against env.mat: per block of
        `batch_users` users one catalogue sweep over dataset_val.df_photo_env (device_model().sweep: Pairwise, the IPS / PD builds, DICE) and one
        row-wise top-k (cirs_rows_topk), then one cirs_rank_metrics over all lists.  Returns the dict of RankMetrics.evaluate; its "ids" entry holds
        the lists [n, k] (env-encoded: positions in df_photo_env, as recommend_k_item returns them).  rel_threshold is required."""
        from cirs_hip.rankmetrics import RankMetrics, check_k
        k = check_k(k)
        df_item_val = dataset_val.df_photo_env
        item_index = df_item_val.index.to_numpy()
        assert np.array_equal(item_index, np.asarray(env.lbe_photo.classes_)), "df_photo_env must be in env item order (lbe_photo.classes_)"
        dm = self.device_model()
        rm = RankMetrics.for_env(env, rel_threshold=rel_threshold, device=dm.device)
        users = np.arange(env.mat.shape[0]) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
        if len(users) and (users.min() < 0 or users.max() >= env.mat.shape[0]):
            raise ValueError(f"users must be env user ids in [0, {env.mat.shape[0]})")
        raw_users = np.asarray(env.lbe_user.classes_)[users]
        feats = df_item_val[["feat0", "feat1", "feat2", "feat3"]].to_numpy()
        dur = df_item_val["photo_duration"].to_numpy()
        step = max(1, int(batch_users))
        ids = torch.empty((len(users), k), dtype=torch.int64, device=dm.device)
        for u0 in range(0, len(users), step):
            scores, _ = dm.sweep(raw_users[u0:u0 + step], item_index, feats, dur)       # [block, I] fp32 on the device
            ids[u0:u0 + step] = rm.topk_rows(scores, k)[0]
        out = rm.evaluate(ids, users)
        out["ids"] = ids
        return out

    # ---- static-baseline recommendation (reference core/user_model.py:250-348) ------------------------------------------
    def compile_UCB(self, n_arm):
        self.n_rec = n_arm
        self.n_each = np.ones(n_arm)

    def recommend_k_item(self, user, dataset_val, k=1, is_softmax=True, epsilon=0, is_ucb=False, recommended_ids=[], gumbel=None,
                         seed=None):
        """One catalogue sweep for `user` (original id) over dataset_val.df_photo_env, then the choice of k items on the device
        (cirs_select_items).  Returns (recommended_id_transform, recommended_id_raw, value_rec) like the reference (core/user_model.py:254-346):
        positions in df_photo_env, original ids, u_value of the picks.
        k > 1: `torch.multinomial(softmax, k, replacement=False)` draws item after item from the renormalised rest and `torch.topk` is a
        repeated arg-max -- both are k selections with the already chosen items removed, which is how they run here (k launches of the
        selection kernel over the same scores; with harness noise `gumbel` the k picks are the Gumbel top-k of logit + noise, i.e. one
        sample without replacement).  The epsilon-greedy branch replaces all k picks by uniform draws (with repetition, like
        `torch.randint(0, n, (k,))`)."""
        from cirs_hip.static_policy import select_items
        df_item_val = dataset_val.df_photo_env
        item_index = df_item_val.index.to_numpy()
        I = len(item_index)
        assert 1 <= k <= I - len(recommended_ids), "k exceeds the number of items left"
        dm = self.device_model()
        feats = df_item_val[["feat0", "feat1", "feat2", "feat3"]].to_numpy()
        dur = df_item_val["photo_duration"].to_numpy()
        pred, _ = dm.sweep(np.asarray([user]), item_index, feats, dur)          # [1, I] on the device
        words = np.zeros((I + 31) // 32, dtype=np.uint32)
        if len(recommended_ids):
            ids = np.asarray(recommended_ids, dtype=np.int64)
            np.bitwise_or.at(words, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
        bonus = None
        if is_ucb and len(recommended_ids) == 0:
            if not hasattr(self, "n_rec"):
                self.compile_UCB(I)
            bonus = torch.as_tensor(((2 * np.log(self.n_rec) / self.n_each) ** 0.5).astype(np.float32))
        explore = k > 1 and epsilon > 0 and np.random.random() < epsilon     # k = 1: the kernel's own epsilon draw (bit-exact vs the oracle)
        picks, vals = [], []
        for i in range(k):
            self._rec_calls = getattr(self, "_rec_calls", 0) + 1
            visited = torch.as_tensor(words.view(np.int32)).reshape(1, -1) if (len(recommended_ids) or i > 0) else None
            act, val = select_items(pred, softmax=is_softmax, bonus=bonus, visited=visited,
                                    epsilon=float(epsilon) if k == 1 else (1.0 if explore else 0.0), gumbel=gumbel,
                                    seed=self.seed_rec if seed is None else seed, rng_step=self._rec_calls)
            a = int(act.cpu()[0])
            picks.append(a); vals.append(float(val.cpu()[0]))
            if not explore:
                words[a >> 5] |= np.uint32(1) << np.uint32(a & 31)
        recommended_id_transform = np.asarray(picks, dtype=np.int64)
        if is_ucb:
            self.n_rec += k
            self.n_each[recommended_id_transform] += 1
        return recommended_id_transform, item_index[recommended_id_transform], np.asarray(vals, dtype=np.float32)

