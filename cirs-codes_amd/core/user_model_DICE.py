"""UserModel_DICE (reference core/user_model_DICE.py:15-192): the DICE debiasing baseline -- a main DeepFM over interest and conformity
embeddings of user and item and a second DeepFM shared by the interest pair and the conformity pair -- trained and evaluated on the
device (cirs_hip.dice_train: cirs_dice_train_epoch, cirs_dice_forward).

Constructor call, state_dict names and shapes are the reference's, so its checkpoints load.  recommend_k_item comes from
core.user_model.UserModel and runs over device_model() (cirs_hip.dice_train.DeviceDice); so do compile_RL_test, fit_data, predict_data and
evaluate_data (the trainer is cirs_hip.dice_train.DiceTrainer, the validation pass cirs_dice_validate)."""
import torch
from torch import nn

from core.inputs import SparseFeatP
from core.user_model import UserModel
from deepctr_torch.inputs import DenseFeat, build_input_features

_sigmoid = nn.Sigmoid()


def loss_kuaishou_DICE(y, y_deepfm_pos, y_deepfm_neg, y_deepfm_pos_int, y_deepfm_neg_int, y_deepfm_pos_con, y_deepfm_neg_con, score):
    """DICE.py:273-286: regression + click BPR on the main network, conformity BPR signed by the score (+1: the positive is the more
    popular item), interest BPR on the rows where the negative is the more popular one.  The torch formula is for host use;
    UserModel_DICE.fit_data recognises the loss by its `loss_kind` and runs it inside cirs_dice_train_epoch."""
    loss_y = ((y_deepfm_pos - y) ** 2).mean()
    bpr_click = -_sigmoid(y_deepfm_pos - y_deepfm_neg).log().mean()
    bpr_con = -(_sigmoid(y_deepfm_pos_con - y_deepfm_neg_con).log() * score).mean()
    bpr_int = -(_sigmoid(y_deepfm_pos_int - y_deepfm_neg_int).log() * (score < 0)).mean()
    return loss_y + bpr_click + bpr_con + bpr_int


loss_kuaishou_DICE.loss_kind = "dice"


def _linear(columns, init_std, g):
    """core/layers.py:20-41: one [V, 1] table per embedding name and one weight row per dense column."""
    m = nn.Module()
    names = {}
    for f in columns:
        if isinstance(f, SparseFeatP):
            names.setdefault(f.embedding_name, f)
    m.embedding_dict = nn.ModuleDict({k: nn.Embedding(int(f.vocabulary_size), 1) for k, f in names.items()})
    for e in m.embedding_dict.values():
        with torch.no_grad():
            e.weight.copy_(torch.randn(e.weight.shape, generator=g) * init_std)
    n_dense = sum(f.dimension for f in columns if isinstance(f, DenseFeat))
    if n_dense:
        m.weight = nn.Parameter(torch.randn(n_dense, 1, generator=g) * init_std)
    return m


def _tower(k_in):
    dnn = nn.Module()
    dnn.linears = nn.ModuleList([nn.Linear(k_in, 64), nn.Linear(64, 64)])
    out = nn.Module()
    out.bias = nn.Parameter(torch.zeros(1, 1))
    return dnn, nn.Linear(64, 1, bias=False), out


class UserModel_DICE(UserModel):
    def __init__(self, feature_columns, y_columns, task, task_logit_dim, dnn_hidden_units=(128, 128), l2_reg_embedding=1e-5, l2_reg_dnn=1e-1,
                 init_std=0.0001, task_dnn_units=None, seed=2021, dnn_dropout=0, dnn_activation="relu", dnn_use_bn=False, device="cpu",
                 padding_idx=None, l2_reg_linear=1e-5):
        super().__init__()
        assert task == "regression" and task_logit_dim == 1 and tuple(dnn_hidden_units) == (64, 64), \
            "the device model is the script's: one regression task, dnn_hidden_units (64, 64)"
        assert task_dnn_units is None and not dnn_use_bn and dnn_dropout == 0 and dnn_activation == "relu"
        assert len(feature_columns) == 16, "the 16 columns of load_dataset_kuaishou_DICE"
        self.feature_columns, self.y_columns = feature_columns, y_columns
        self.task, self.task_logit_dim = task, task_logit_dim
        self.feature_index = build_input_features(feature_columns)
        self.device = device
        self.feature_main = feature_columns[:9]
        self.feature_ui_int = [feature_columns[0], feature_columns[2]]
        self.feature_ui_con = [feature_columns[1], feature_columns[3]]
        g = torch.Generator().manual_seed(seed)
        names = {}
        for f in feature_columns:
            if isinstance(f, SparseFeatP):
                names.setdefault(f.embedding_name, f)
        assert list(names) == ["user_int", "user_con", "photo_int", "photo_con", "feat"], list(names)
        E = int(names["feat"].embedding_dim)
        assert all(int(f.embedding_dim) == E for f in names.values()), "entity_dim == feature_dim"
        self.embedding_dict = nn.ModuleDict({k: nn.Embedding(int(f.vocabulary_size), E) for k, f in names.items()})
        with torch.no_grad():
            for e in self.embedding_dict.values():
                e.weight.copy_(torch.randn(e.weight.shape, generator=g) * init_std)
            self.embedding_dict["feat"].weight[0] = 0        # padding_idx = 0
        self.linear_model = _linear(feature_columns, init_std, g)        # the base class's copy: unused in the forward, still regularised
        self.dnn_main, self.last_main, self.out_main = _tower(8 * E + 1)
        self.dnn_ui, self.last_ui, self.out_ui = _tower(2 * E)
        self.linear_main = _linear(self.feature_main, init_std, g)
        self.linear_ui = _linear(self.feature_ui_int, init_std, g)
        self._l2 = (float(l2_reg_embedding), float(l2_reg_linear), float(l2_reg_dnn))
        self._dev = None
        self._trainer = None
        self.optim = None
        self.RL_eval_fun = None

    # ---- evaluation ---------------------------------------------------------------------------------------------------------
    def device_model(self):
        """DeviceDice over the current weights (rebuilt after load_state_dict / fit_data)."""
        if self._dev is None:
            from cirs_hip.dice_train import DeviceDice
            self._dev = DeviceDice(self.state_dict())
        return self._dev

    def load_state_dict(self, state_dict, strict=True):
        self._dev = None
        self._trainer = None       # the Adam moments belong to the parameters they were fitted on
        return super().load_state_dict(state_dict, strict=strict)

    def forward(self, x, score=None):
        """x: float tensor (n, 7) = [user_id, photo_id, feat0..3, photo_duration] carrying raw ids; the ids stand in both of their
        columns (core/user_model_DICE.py:189-192)."""
        x = torch.as_tensor(x)
        ids = x[:, :6].long()
        y = self.device_model().forward(ids[:, 0], ids[:, 1], ids[:, 2:6].int(), x[:, 6].float()).unsqueeze(1)
        return y if score is None else y * torch.as_tensor(score).to(y.device, y.dtype)

    # ---- training (reference core/user_model.py:71-170) -----------------------------------------------------------------------
    def compile(self, optimizer, loss_dict=None, metrics=None, metric_fun=None, loss_func=None):
        assert optimizer == "adam" or isinstance(optimizer, torch.optim.Adam), "the device step implements torch.optim.Adam"
        assert getattr(loss_func, "loss_kind", None) == "dice", \
            "pass core.user_model_DICE.loss_kuaishou_DICE: the loss runs inside the device training step"
        self.metrics_names = ["loss"]
        self.loss_func, self.metric_fun, self.metrics = loss_func, metric_fun, metrics
        self.optim = "adam"
        self._lr = optimizer.param_groups[0]["lr"] if isinstance(optimizer, torch.optim.Adam) else 1e-3

    def _new_trainer(self):
        from cirs_hip.dice_train import DiceTrainer
        return DiceTrainer(self.state_dict(), l2_embedding=self._l2[0], l2_linear=self._l2[1], l2_all=self._l2[2], lr=self._lr)

    _loss_columns = (0, 5)      # {loss, reg_loss} of cirs_dice_train_epoch's per-step rows; fit_data itself is the base class's
