"""Evaluation callbacks of the CIRS protocol on device trajectories (reference evaluation.py).

  get_feat_dominate_dict   evaluation.py:10-77  ("ifeat_feat": share of recommendations carrying a dominating category)
  Callback_Coverage_Count  evaluation.py:286-371 (CV, CV_turn and ifeat_* for the FB / NX_0 / NX_k test collectors)
  test_kuaishou            evaluation.py:179-234  (the per-epoch evaluation loop of the LinUCB baseline, core/policy/linucb.py)
  test_taobao              evaluation.py:238-282  (the VirtualTaobao static baselines: MLP-taobao.py, MLP-epsilonGreedy-taobao.py)
  test_ranking_kuaishou    no reference counterpart (offline Precision / Recall / HR / MRR / NDCG / ILD / CV @k of a static model's top-k lists)

The reference walks the replay buffers on the host (buffer.prev / buffer.next); here each collector's buffer carries the
device trajectory of its fused rollout and the counts come from cirs_eval_coverage (integer kernel, bit-exact)."""
import numpy as np
import torch

from cirs_hip.evalmetrics import CoverageCounter, dominated_values, item_flags


def _feat_columns(df_item_val):
    return [c for c in df_item_val.columns if str(c).startswith("feat")]  # .filter(regex="^feat", axis=1)


def get_feat_dominate_dict(df_item_val, all_acts_origin, item_feat_domination, top_rate=0.6):
    """Same contract as the reference: df_item_val is indexed by the ORIGINAL item ids, all_acts_origin are original ids."""
    if item_feat_domination is None:  # for yahoo
        return dict()
    out = {}
    pos = df_item_val.index.get_indexer(np.asarray(all_acts_origin))
    assert (pos >= 0).all(), "recommended item missing from df_item_val"
    counter = CoverageCounter(len(df_item_val))
    if "feat" in item_feat_domination:  # kuairec / kuairand: multi-hot categories in the feat* columns
        flags = item_flags(df_item_val[_feat_columns(df_item_val)].to_numpy(), dominated_values(item_feat_domination["feat"], top_rate))
        _, n, fl = counter.count(torch.as_tensor(pos), torch.as_tensor(flags))
        out["ifeat_feat"] = fl / n
    else:  # coat: one column per feature
        for feat_name, sorted_items in item_feat_domination.items():
            flags = item_flags(df_item_val[[feat_name]].to_numpy(), dominated_values(sorted_items, top_rate))
            _, n, fl = counter.count(torch.as_tensor(pos), torch.as_tensor(flags))
            out["ifeat_" + feat_name] = fl / n
    return out


def interactive_evaluation(model, env, dataset_val, is_softmax, epsilon, is_ucb, k, need_transform, num_trajectory, item_feat_domination,
                           remove_recommended, force_length=0, top_rate=0.6, users=None, seed=0):
    """reference evaluation.py:79-151 with the num_trajectory trajectories run in LOCK-STEP on the device: one catalogue
    sweep per trajectory user (the model is static), then per step cirs_select_items -> env step (cirs_rollout_static).
    Same result dict.  With is_ucb the arm counts change after every single recommendation of every trajectory
    (core/user_model.py:303-314, 340-342): that path runs the trajectories one after the other, one device step per
    recommendation (_interactive_evaluation_ucb).  Users can be supplied (the reference draws them with the unseeded `random`)."""
    from cirs_hip.evalmetrics import CoverageCounter
    from cirs_hip.static_policy import StaticRollout
    assert k == 1 and need_transform, "built for KuaishouEnv (need_transform=True, k=1)"
    B = int(num_trajectory)
    df_item_val = dataset_val.df_photo_env
    item_index = df_item_val.index.to_numpy()
    assert np.array_equal(item_index, np.asarray(env.lbe_photo.classes_)), "df_photo_env must be in env item order (lbe_photo.classes_)"
    I = len(item_index)
    dev_env = env.build_device_env(B)
    if users is None:
        users = np.random.randint(0, env.mat.shape[0], B)
    users = np.asarray(users)
    raw_users = np.asarray(env.lbe_user.classes_)[users]
    feats = df_item_val[["feat0", "feat1", "feat2", "feat3"]].to_numpy()
    dur = df_item_val["photo_duration"].to_numpy()
    scores, _ = model.device_model().sweep(raw_users, item_index, feats, dur)   # [B, I] u_value of every trajectory user
    ro = StaticRollout(dev_env)
    T = dev_env.max_turn if force_length <= 0 else min(force_length, dev_env.max_turn)
    if is_ucb:
        return _interactive_evaluation_ucb(model, env, dataset_val, is_softmax, epsilon, B, item_feat_domination, remove_recommended,
                                           force_length, top_rate, users, raw_users, item_index, feats, dur, seed)
    ro.run(torch.as_tensor(users), scores, softmax=is_softmax, epsilon=epsilon, seed=seed, remove_recommended=remove_recommended,
           force_length=force_length, n_steps=T)
    valid = ro.act >= 0
    total_turns = int(valid.sum())
    cumulative_reward = float((ro.rew * valid).sum())
    total_click_loss = float(((ro.value.double() - ro.rew).abs() * valid).sum())
    ctr = cumulative_reward / total_turns
    click_loss = total_click_loss / total_turns
    cc = CoverageCounter(I, device=ro.act.device)
    flags = None
    if item_feat_domination is not None and "feat" in item_feat_domination:
        flags = torch.as_tensor(item_flags(feats, dominated_values(item_feat_domination["feat"], top_rate)))
    hit_item, n_acts, n_fl = cc.count(ro.act, flags)
    eval_result_RL = {"click_loss": click_loss, "CV": f"{hit_item / I:.5f}", "CV_turn": f"{hit_item / n_acts:.5f}", "ctr": ctr,
                      "len_tra": total_turns / B, "R_tra": cumulative_reward / B}
    if flags is not None:
        eval_result_RL["ifeat_feat"] = n_fl / n_acts
    if remove_recommended:
        eval_result_RL = {f"NX_{force_length}_" + key: v for key, v in eval_result_RL.items()}
    interactive_evaluation.last_rollout = ro
    return eval_result_RL


def _interactive_evaluation_ucb(model, env, dataset_val, is_softmax, epsilon, B, item_feat_domination, remove_recommended, force_length,
                                top_rate, users, raw_users, item_index, feats, dur, seed):
    """is_ucb=True (reference evaluation.py:87-120 with core/user_model.py:303-314, 340-342): the bonus sqrt(2 ln n_rec / n_each) is
    added to u_value when nothing is excluded (recommended_ids == [], i.e. always without remove_recommended, only at the first step
    of a trajectory with it), and (n_rec, n_each) change after EVERY recommendation -- sequential by construction: trajectories one
    after the other on a 1-env device env, one cirs_rollout_static step per recommendation, counts kept on the model like the
    reference's.  reward_pred (click_loss) includes the bonus when it was applied, as in the reference (value_rec = u_value[...])."""
    from cirs_hip.evalmetrics import CoverageCounter
    from cirs_hip.static_policy import StaticRollout
    I = len(item_index)
    dev_env = env.build_device_env(1)
    ro = StaticRollout(dev_env)
    T = dev_env.max_turn if force_length <= 0 else min(force_length, dev_env.max_turn)
    if not hasattr(model, "n_rec"):
        model.compile_UCB(I)
    total_turns, cumulative_reward, total_click_loss = 0, 0.0, 0.0
    all_acts = []
    for i in range(B):
        scores, _ = model.device_model().sweep(raw_users[i:i + 1], item_index, feats, dur)   # [1, I]
        ro.begin(torch.as_tensor(users[i:i + 1]), remove_recommended)
        n_acts = 0
        for t in range(T):
            bonus = None
            if not remove_recommended or n_acts == 0:
                bonus = torch.as_tensor(((2 * np.log(model.n_rec) / model.n_each) ** 0.5).astype(np.float32))
            ro.step(t, scores, softmax=is_softmax, epsilon=epsilon, seed=seed, rng_base=i * dev_env.max_turn, force_length=force_length,
                    bonus=bonus)
            a = int(ro.act[t, 0])
            if a < 0:
                break
            model.n_rec += 1
            model.n_each[a] += 1
            n_acts += 1
            all_acts.append(a)
            r = float(ro.rew[t, 0])
            total_turns += 1
            cumulative_reward += r
            total_click_loss += abs(float(ro.value[t, 0]) - r)
            if bool(ro.done[t, 0]):
                break
    ctr = cumulative_reward / total_turns
    click_loss = total_click_loss / total_turns
    acts = torch.as_tensor(np.asarray(all_acts, dtype=np.int64))
    cc = CoverageCounter(I)
    flags = None
    if item_feat_domination is not None and "feat" in item_feat_domination:
        flags = torch.as_tensor(item_flags(feats, dominated_values(item_feat_domination["feat"], top_rate)))
    hit_item, n_acts_all, n_fl = cc.count(acts, flags)
    res = {"click_loss": click_loss, "CV": f"{hit_item / I:.5f}", "CV_turn": f"{hit_item / n_acts_all:.5f}", "ctr": ctr,
           "len_tra": total_turns / B, "R_tra": cumulative_reward / B}
    if flags is not None:
        res["ifeat_feat"] = n_fl / n_acts_all
    if remove_recommended:
        res = {f"NX_{force_length}_" + key: v for key, v in res.items()}
    return res


def test_static_model_in_RL_env(model, env, dataset_val, is_softmax=True, epsilon=0, is_ucb=False, k=1, need_transform=False,
                                num_trajectory=100, item_feat_domination=None, force_length=10, top_rate=0.6, users=None, seed=0):
    """reference evaluation.py:153-176: free browsing, no-overlap, no-overlap with forced length."""
    out = {}
    for remove, fl in ((False, 0), (True, 0), (True, force_length)):
        out.update(interactive_evaluation(model, env, dataset_val, is_softmax, epsilon, is_ucb, k, need_transform, num_trajectory,
                                          item_feat_domination, remove_recommended=remove, force_length=fl, top_rate=top_rate, users=users,
                                          seed=seed))
    return out


test_static_model_in_RL_env.__test__ = False  # not a pytest test


def test_kuaishou(model, env, dataset_val, is_softmax=True, epsilon=0, is_ucb=False, *, users=None, num_trajectory=200):
    """reference evaluation.py:179-234 for a model that keeps the device LinUCB state (core.policy.linucb.linucb_policy): the
    num_trajectory trajectories in LOCK-STEP.  The model does not change during the loop, so a trajectory recommends the same item at
    every step until the env's exit rule ends it: one scoring launch gives every trajectory user its item and the predicted reward
    (recommend_k_item for all of them at once), then one cirs_rollout_static plays the trajectories, the item handed over as a [B, I]
    indicator matrix of scores.  click_loss comes from the returned means against the trajectory rewards in float64.  Same result
    dict.  `users` (env numbering) can be supplied; the reference draws them inside env.reset() with the unseeded `random`."""
    from cirs_hip.static_policy import StaticRollout
    state = getattr(model, "device_state", None)
    if state is None:
        raise TypeError("test_kuaishou plays a model with the device LinUCB state (core.policy.linucb.linucb_policy)")
    if epsilon != 0 or is_ucb:
        raise ValueError("test_kuaishou: the LinUCB policy explores through its own upper confidence bound: epsilon must be 0 and is_ucb False")
    df_item_val = dataset_val.df_photo_env
    item_index = df_item_val.index.to_numpy()
    assert np.array_equal(item_index, np.asarray(env.lbe_photo.classes_)), "df_photo_env must be in env item order (lbe_photo.classes_)"
    I = len(item_index)
    if users is None:
        users = np.random.randint(0, env.mat.shape[0], int(num_trajectory))
    users = np.asarray(users)
    B = len(users)
    raw_users = np.asarray(env.lbe_user.classes_)[users]
    best, mean = state.score(raw_users.astype(np.float64), df_item_val.to_numpy())       # [B] arm (= env item id), [B] theta^T x
    dev_env = env.build_device_env(B)
    scores = torch.zeros((B, I), dtype=torch.float32, device=dev_env.device)
    scores[torch.arange(B, device=dev_env.device), best.to(dev_env.device)] = 1.0
    ro = StaticRollout(dev_env)
    ro.run(torch.as_tensor(users), scores, softmax=False)
    valid = ro.act >= 0
    total_turns = int(valid.sum())
    cumulative_reward = float((ro.rew * valid).sum())
    total_click_loss = float(((mean.to(ro.rew.device)[None, :] - ro.rew).abs() * valid).sum())
    hit_item, n_acts, _ = CoverageCounter(I, device=ro.act.device).count(ro.act, None)
    test_kuaishou.last_rollout = ro
    return {"click_loss": total_click_loss / total_turns, "CV": f"{hit_item / I:.5f}", "CV_turn": f"{hit_item / n_acts:.5f}",
            "ctr": cumulative_reward / total_turns, "len_tra": total_turns / B, "R_tra": cumulative_reward / B}


test_kuaishou.__test__ = False  # not a pytest test


def test_ranking_kuaishou(model, env, dataset_val, k=10, *, rel_threshold=None, users=None):
    """Offline ranking evaluation of a static user model (UserModel.evaluate_ranking: Pairwise, IPS / PD, DICE) against the fully observed
    KuaishouEnv matrix: {"Precision@k", "Recall@k", "HR@k", "MRR@k", "NDCG@k", "ILD@k", "CV@k", "n", "per_row", "ids"}.  rel_threshold is
    required.  Like the other evaluation functions it can be handed to compile_RL_test through functools.partial (env, dataset_val, k and
    rel_threshold bound).  No reference counterpart."""
    return model.evaluate_ranking(env, dataset_val, k, rel_threshold=rel_threshold, users=users)


test_ranking_kuaishou.__test__ = False  # not a pytest test


def test_taobao(model, env, epsilon=0, *, device=None, num_trajectory=100, seed=0):
    """reference evaluation.py:238-282: `model` (two-task UserModel_MMOE: static state 91 -> 27 item features + click prediction)
    plays num_trajectory trajectories against `env`, a VirtualTB in static-state mode -> {"ctr", "click_loss", "len_tra", "R_tra"}.

    device=None: the reference's procedure on the host, statement for statement, so torch's and numpy's global generators are consumed
    as the reference consumes them (the epsilon draw only when epsilon > 0; the exploration action is np.random.random(27); the action is
    the raw prediction, not clipped to the action box).  device="cuda": every trajectory in lock step inside one launch
    (cirs_hip.vtb_static.DeviceVtbStaticEval; counter-based noise keyed by `seed`, env weights and exit-rule settings read off `env`)."""
    if not getattr(env, "static", False):
        raise ValueError("test_taobao plays the static baselines: the env must be in static-state mode (env.set_state_mode(True)); the "
                         "policy's 91 inputs are the static state [user | last clicks, last second draw | turn]")
    if device is not None:
        from cirs_hip.vtb_static import DeviceVtbStaticEval
        return DeviceVtbStaticEval(env, model, num_trajectory, seed=seed, device=device).run(epsilon)
    cumulative_reward = 0
    total_click_loss = 0
    total_turns = 0
    for i in range(num_trajectory):
        features = env.reset()
        done = False
        while not done:
            res = model(torch.FloatTensor(features).to(model.device).unsqueeze(0)).to("cpu").squeeze()
            item_feat_predict = res[model.y_index["feat_item"][0]:model.y_index["feat_item"][1]]
            action = item_feat_predict.detach().numpy()
            if epsilon > 0 and np.random.random() < epsilon:
                action = np.random.random(action.shape)
            reward_pred = res[model.y_index["y"][0]:model.y_index["y"][1]]
            features, reward, done, info = env.step(action)
            total_turns += 1
            cumulative_reward += reward
            total_click_loss += np.absolute(float(reward_pred.detach().numpy().reshape(-1)[0]) - reward)
    ctr = cumulative_reward / total_turns
    click_loss = total_click_loss / total_turns
    return {"ctr": ctr, "click_loss": click_loss, "len_tra": total_turns / num_trajectory, "R_tra": cumulative_reward / num_trajectory}


test_taobao.__test__ = False  # not a pytest test


class Callback_Coverage_Count:
    def __init__(self, test_collector_set, df_item_val, need_transform, item_feat_domination, lbe_photo, top_rate):
        self.collector_dict = test_collector_set.collector_dict
        self.num_items = test_collector_set.env.mat[0].shape[1]
        self.df_item_val = df_item_val
        self.need_transform = need_transform
        self.item_feat_domination = item_feat_domination
        self.lbe_photo = lbe_photo
        self.top_rate = top_rate
        self._counter = None
        self._flags = {}
        if item_feat_domination is not None:
            # flags per ENV item id: env id -> original id (lbe_photo.inverse_transform == classes_[id]) -> df_item_val row
            ids = np.arange(self.num_items)
            # LabelEncoder.inverse_transform(ids) == classes_[ids]
            origin = (self.lbe_photo.inverse_transform(ids) if hasattr(self.lbe_photo, "inverse_transform")
                      else np.asarray(self.lbe_photo.classes_)[ids]) if need_transform else ids
            rows = df_item_val.loc[origin]
            if "feat" in item_feat_domination:
                self._flags["ifeat_feat"] = item_flags(rows[_feat_columns(rows)].to_numpy(), dominated_values(item_feat_domination["feat"], top_rate))
            else:
                for feat_name, sorted_items in item_feat_domination.items():
                    self._flags["ifeat_" + feat_name] = item_flags(rows[[feat_name]].to_numpy(), dominated_values(sorted_items, top_rate))

    def on_epoch_begin(self, epoch):
        pass

    def on_train_begin(self):
        pass

    def on_train_end(self):
        pass

    def on_epoch_end(self, epoch, results=None, **kwargs):
        results_all = {}
        for name, collector in self.collector_dict.items():
            ro = getattr(collector.buffer, "_rollout", None)
            assert ro is not None, "collector has not collected yet"
            act = ro.traj.act  # [T, B] int64 on the device, -1 once an env has finished
            if self._counter is None:
                self._counter = CoverageCounter(self.num_items, device=act.device)
                self._flags = {k: torch.as_tensor(v).to(act.device) for k, v in self._flags.items()}
            res = {}
            hit = n = None
            for key, fl in (self._flags or {None: None}).items():
                hit, n, n_fl = self._counter.count(act, fl)
                if key is not None:
                    res[key] = n_fl / n
            res["CV"] = hit / self.num_items
            res["CV_turn"] = hit / n
            results_all.update({name + "_" + k: v for k, v in res.items()} if name != "FB" else res)
        results.update(results_all)
        return results
