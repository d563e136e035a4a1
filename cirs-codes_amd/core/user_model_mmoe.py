"""UserModel_MMOE (reference core/user_model_mmoe.py:15-262 over core/layers.py MMOELayer/Linear and DeepCTR-Torch's DNN /
PredictionLayer): the user model of the VirtualTaobao experiments (CIRS-UserModel-taobao.py:100-148) -- BASELINE configs[0], CPU
plumbing.  Parameters under the reference's state_dict names; `forward` is plain torch on whatever device the module lives on (this
is not a hot path: one 1 x 118 row per env step); `compile` / `fit_data` train on the device (cirs_hip.mmoe_train.MMoETrainer:
cirs_mmoe_train_epoch, two launches per optimiser step, loss_taobao inside the kernel).  The two-task build of the static baselines
(MLP-taobao.py, MLP-epsilonGreedy-taobao.py: 91 static-state inputs -> feat_item (27) and y (1)) trains the same way behind the marker
loss_taobao_mlp (cirs_hip.mmoe_train.MlpTrainer: cirs_mlp_train_epoch); `compile_RL_test` is the reference's per-epoch evaluation hook.

    y_task = PredictionLayer_task( Linear_task(X)  [+ FM over the sparse embeddings, none for the all-dense Taobao features]
                                   + tower_task( MMoE_task( DNN(X) ) ) )
    MMoE: experts = Linear(H, n_experts * expert_dim) reshaped [B, expert_dim, n_experts]; gate_task = softmax(Linear(H, n_experts,
    no bias)); output = experts @ gate."""
import torch
from torch import nn

from core.inputs import compute_input_dim
from core.user_model import UserModel
from deepctr_torch.inputs import DenseFeat, build_input_features


def loss_taobao(y_predict=None, y_true=None, exposure=None, y_index=None):
    """Marker of the reference's loss (CIRS-UserModel-taobao.py:185-191), mean((y_predict / (1 + exposure) - y)^2 (y + 1)): pass it to
    UserModel_MMOE.compile; the loss itself runs inside cirs_mmoe_train_step."""
    raise RuntimeError("loss_taobao is evaluated on the device by cirs_mmoe_train_step; it is a marker for UserModel_MMOE.compile")


loss_taobao.device_loss = "taobao"


def loss_taobao_mlp(y_predict=None, y_true=None, exposure=None, y_index=None):
    """Marker of the static baselines' loss (MLP-taobao.py:137-155), mse(click * feat_item) + mse(y) with click = y_true[:, -1]: pass it
    to UserModel_MMOE.compile of the two-task build; the loss itself runs inside cirs_mlp_train_step."""
    raise RuntimeError("loss_taobao_mlp is evaluated on the device by cirs_mlp_train_step; it is a marker for UserModel_MMOE.compile")


loss_taobao_mlp.device_loss = "taobao_mlp"


class _Dense(nn.Module):
    """DeepCTR DNN without batch-norm / dropout (dnn_use_bn=False, dnn_dropout=0): `linears.<i>`, ReLU after every layer."""

    def __init__(self, d_in, hidden):
        super().__init__()
        dims = [d_in] + list(hidden)
        self.linears = nn.ModuleList([nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])

    def forward(self, x):
        for lin in self.linears:
            x = torch.relu(lin(x))
        return x


class _MMoE(nn.Module):
    def __init__(self, d_in, num_tasks, num_experts, out_dim):
        super().__init__()
        self.num_experts, self.out_dim = num_experts, out_dim
        self.expert_network = nn.Linear(d_in, num_experts * out_dim, bias=True)
        self.gating_networks = nn.ModuleList([nn.Linear(d_in, num_experts, bias=False) for _ in range(num_tasks)])
        for m in (self.expert_network, *self.gating_networks):
            nn.init.normal_(m.weight)

    def forward(self, x):
        experts = self.expert_network(x).reshape(-1, self.out_dim, self.num_experts)
        return [torch.bmm(experts, gate(x).softmax(1).unsqueeze(-1)).squeeze() for gate in self.gating_networks]


class _DenseLinear(nn.Module):
    """core/layers.py Linear for all-dense feature columns: X[:, dense columns] @ weight."""

    def __init__(self, n_dense):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n_dense, 1))

    def forward(self, x_dense):
        return x_dense.matmul(self.weight)


class _Bias(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros((1, dim)))


class UserModel_MMOE(UserModel):
    def __init__(self, feature_columns, y_columns, num_tasks, tasks, task_logit_dim, num_experts=4, expert_dim=8,
                 dnn_hidden_units=(128, 128), l2_reg_embedding=1e-5, l2_reg_dnn=1e-2, init_std=0.0001, task_dnn_units=None, seed=2021,
                 dnn_dropout=0, dnn_activation="relu", dnn_use_bn=False, device="cpu", padding_idx=None, ab_columns=None):
        super().__init__()
        assert all(isinstance(f, DenseFeat) for f in feature_columns), "the Taobao user model has dense features only (CIRS-UserModel-taobao.py:100)"
        assert dnn_activation == "relu" and not dnn_use_bn and dnn_dropout == 0 and task_dnn_units is None and ab_columns is None
        assert all(v == "regression" for v in tasks.values()), "regression tasks only"
        torch.manual_seed(seed)
        self.feature_columns, self.y_columns, self.tasks, self.task_logit_dim = feature_columns, y_columns, tasks, task_logit_dim
        self.feature_index = build_input_features(feature_columns)
        self.y_index = build_input_features(y_columns)
        self.device = device
        d_in = compute_input_dim(feature_columns)
        self.linear_model = _DenseLinear(d_in)                     # base-class duplicate, unused by forward (as in the reference)
        self.dnn = _Dense(d_in, dnn_hidden_units)
        for lin in self.dnn.linears:
            nn.init.normal_(lin.weight, mean=0, std=init_std)
        self.mmoe_layer = _MMoE(dnn_hidden_units[-1], num_tasks, num_experts, expert_dim)
        self.tower_network = nn.ModuleList([nn.Linear(expert_dim, dim, bias=False) for dim in task_logit_dim.values()])
        self.out = nn.ModuleList([_Bias(dim) for dim in task_logit_dim.values()])
        self.linear_model_task = nn.ModuleList([_DenseLinear(d_in) if dim == 1 else None for dim in task_logit_dim.values()])
        for m in [self.linear_model] + [m for m in self.linear_model_task if m is not None]:
            nn.init.normal_(m.weight, mean=0, std=init_std)
        self.to(device)
        self._l2 = (1e-5, float(l2_reg_dnn))     # (linear_model: the base class's l2_reg_linear default, every parameter)
        self.optim = None
        self._trainer = None
        self._kind = None                        # which device step compile() selected: "taobao" (one task) or "taobao_mlp" (two tasks)
        self.RL_eval_fun = None

    # ---- training (reference core/user_model.py:74-170 with loss_taobao) ------------------------------------------------------
    def compile(self, optimizer, loss_dict=None, metrics=None, metric_fun=None, loss_func=None):
        if not (optimizer == "adam" or isinstance(optimizer, torch.optim.Adam)):
            raise ValueError("the device step implements torch.optim.Adam: pass optimizer=\"adam\" or a torch.optim.Adam instance")
        if getattr(loss_func, "device_loss", None) == "taobao_mlp":
            return self._compile_mlp(optimizer, loss_func, metrics, metric_fun)
        if getattr(loss_func, "device_loss", None) != "taobao":
            raise ValueError("pass core.user_model_mmoe.loss_taobao: the loss runs inside cirs_mmoe_train_step")
        if len(self.tower_network) != 1:
            raise ValueError("loss_taobao trains the build with one regression task; the two-task build of the static baselines "
                             "(feat_item, y) compiles with core.user_model_mmoe.loss_taobao_mlp")
        shape = [tuple(l.weight.shape) for l in self.dnn.linears]
        if len(shape) != 2 or shape[0][1] != 118 or any(s[0] not in (64, 128) for s in shape) or len(self.tower_network) != 1 or \
                self.mmoe_layer.num_experts != 4 or self.mmoe_layer.out_dim != 8 or self.tower_network[0].out_features != 1:
            raise ValueError("the device step trains the VirtualTaobao build only: 118 dense inputs, two hidden layers with widths from "
                             "{64, 128}, 4 experts of dim 8, one regression task of logit dim 1")
        self._compiled("taobao", optimizer, loss_func, metrics, metric_fun)

    def _compiled(self, kind, optimizer, loss_func, metrics, metric_fun):
        """The end of compile() for either build, after its refusals: `kind` selects the device step."""
        self._kind = kind
        self.metrics_names = ["loss"]
        self.loss_func, self.metric_fun, self.metrics = loss_func, metric_fun, metrics
        self.optim = "adam"
        g = optimizer.param_groups[0] if isinstance(optimizer, torch.optim.Adam) else dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        self._adam = dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"])
        self._trainer = None

    def _compile_mlp(self, optimizer, loss_func, metrics, metric_fun):
        """The static baselines' build (MLP-taobao.py:117-124): accepted where the device evaluation accepts it."""
        from cirs_hip.vtb_static import policy_shape
        if len(self.tower_network) != 2:
            raise ValueError("loss_taobao_mlp trains the two-task build of the static baselines (feat_item, y); the build with one "
                             "regression task compiles with core.user_model_mmoe.loss_taobao")
        policy_shape(self)               # ValueError for a shape cirs_vtb_static_eval / cirs_mlp_train_step do not run
        self._compiled("taobao_mlp", optimizer, loss_func, metrics, metric_fun)

    def compile_RL_test(self, RL_eval_fun):
        """reference core/user_model.py:71-72: fit_data evaluates fn(self.eval()) before training and after every epoch."""
        self.RL_eval_fun = RL_eval_fun

    def _publish(self):
        """The trained parameters into the module, under its state_dict names."""
        with torch.no_grad():
            mine = dict(self.named_parameters())
            for k, v in self._trainer.state_dict().items():
                mine[k].copy_(v.reshape(mine[k].shape).to(mine[k].device))

    def fit_data(self, dataset_train, dataset_val=None, batch_size=256, epochs=1, verbose=1, initial_epoch=0, callbacks=None, shuffle=True):
        """One pass per epoch over (x, y, exposure) minibatches, the last one short; an epoch is one cirs_mmoe_train_epoch (two-task
        build: cirs_mlp_train_epoch, y [n, 28], no exposure) call on the device-resident data set.  With compile_RL_test set, the
        evaluation's results join the epoch's logs.  Returns [{"loss": summed total loss / sample count, ...}, ...] like UserModel.fit_data."""
        from cirs_hip.mmoe_train import MlpTrainer, MMoETrainer
        assert self.optim is not None, "call compile() first"
        mlp = self._kind == "taobao_mlp"
        if self._trainer is None:
            self._trainer = (MlpTrainer if mlp else MMoETrainer)(self.state_dict(), l2_linear=self._l2[0], l2_all=self._l2[1], **self._adam)
        tr = self._trainer
        x = torch.as_tensor(dataset_train.x_numpy).to(tr.device, torch.float32).contiguous()
        if mlp:      # y = [27 item features | click]; the score column is not used (MLP-taobao.py:137-155)
            y = torch.as_tensor(dataset_train.y_numpy).to(tr.device, torch.float32).reshape(x.shape[0], -1).contiguous()
            cols = (x, y)
        else:
            y = torch.as_tensor(dataset_train.y_numpy).to(tr.device, torch.float32).reshape(-1).contiguous()
            cols = (x, y, torch.as_tensor(dataset_train.score).to(tr.device, torch.float32).reshape(-1).contiguous())
        n_all = x.shape[0]
        callbacks = callbacks or []
        for cb in callbacks:
            cb.on_train_begin()
        if self.RL_eval_fun:             # core/user_model.py:129-135: the untrained model's evaluation, reported as epoch -1
            logs = {}
            logs.update(self.RL_eval_fun(self.eval()))
            for cb in callbacks:
                cb.on_epoch_end(-1, logs)
        history = []
        for epoch in range(initial_epoch, epochs):
            for cb in callbacks:
                cb.on_epoch_begin(epoch)
            order = torch.randperm(n_all, device=tr.device) if shuffle else torch.arange(n_all, device=tr.device)
            losses = tr.epoch(*cols, order, batch_size)
            logs = {"loss": float(losses.sum(dtype=torch.float64)) / n_all}       # total_loss_epoch / sample_num (core/user_model.py:205)
            if self.RL_eval_fun:         # core/user_model.py:215-219
                self._publish()
                for name, result in self.RL_eval_fun(self.eval()).items():
                    logs[name] = result
            history.append(logs)
            for cb in callbacks:
                cb.on_epoch_end(epoch, logs)
        for cb in callbacks:
            cb.on_train_end()
        self._publish()
        return history

    def load_state_dict(self, state_dict, strict=True):
        self._trainer = None       # the Adam moments belong to the parameters they were fitted on
        return super().load_state_dict(state_dict, strict=strict)

    def forward(self, x):
        x = x.to(torch.float32)
        outs = []
        hidden = self.dnn(x)
        mmoe = self.mmoe_layer(hidden)
        for i, name in enumerate(self.tasks):
            logit = torch.zeros([len(x), self.task_logit_dim[name]], device=x.device)
            if self.linear_model_task[i] is not None:
                logit = logit + self.linear_model_task[i](x)
            logit = logit + self.tower_network[i](mmoe[i])
            outs.append(logit + self.out[i].bias)                  # PredictionLayer("regression"): bias only
        return torch.cat(outs, -1)
