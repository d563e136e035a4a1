"""VtbModel: the one host description of the model the device VirtualTaobao rollout (vtb_rollout.py) and learner (vtb_learn.py) both
run: a HostStateTracker (core/host_rl.py) plus an ActorProb (and its Critic) over a shared Net trunk, CIRS-RL-taobao.py.  What the
device path builds is checked here, cirs_vtb_model_cfg is read off the modules here, and the tensors are enumerated here as ordered
(name, tensor) lists in module registration order: the learner's image layout (make_layout in csrc/vtb_learn.hip), from which the
rollout derives its [in][out] image.  Pure host code: no library needed."""
import ctypes as C

import torch
from torch import nn

from . import abi
from .vtb_host import ACTION_DIM


class ActorKindError(TypeError, ValueError):
    """A non-ActorProb actor: the rollout has always raised TypeError for it, the learner ValueError."""


def stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def u64(x):
    return int(x) & 0xFFFFFFFFFFFFFFFF


def linears(mlp, what):
    """The nn.Linear layers of a tianshou MLP; every other layer must be a ReLU."""
    mods = list(mlp.model)
    for m in mods:
        if not isinstance(m, (nn.Linear, nn.ReLU)):
            raise ValueError(f"{what}: only Linear + ReLU layers are supported by the device rollout and learner, found {type(m).__name__}")
    return [m for m in mods if isinstance(m, nn.Linear)]


def _named(pairs):      # [(name, Linear or LayerNorm)] -> [(name_w, weight), (name_b, bias)] per module
    if any(m.bias is None for _, m in pairs):
        raise ValueError("every Linear of the device rollout and learner needs a bias")
    return [(f"{name}_{k}", p) for name, m in pairs for k, p in (("w", m.weight), ("b", m.bias))]


def tracker_tensors(tracker):
    """ffn_user W b | fnn_gate W b | per layer: in_proj W b, out_proj W b, linear1 W b, linear2 W b, norm1 w b, norm2 w b | decoder W b."""
    out = _named([("user", tracker.ffn_user), ("gate", tracker.fnn_gate)])
    for l, ly in enumerate(tracker.transformer_encoder.layers):
        if getattr(ly, "norm_first", False) or getattr(ly.activation, "__name__", "relu") != "relu":
            raise ValueError("the device rollout and learner build post-norm ReLU TransformerEncoderLayers")
        out += [(f"layer{l}.in_w", ly.self_attn.in_proj_weight), (f"layer{l}.in_b", ly.self_attn.in_proj_bias)]
        out += _named([(f"layer{l}.{k}", m) for k, m in (("out", ly.self_attn.out_proj), ("lin1", ly.linear1), ("lin2", ly.linear2),
                                                         ("norm1", ly.norm1), ("norm2", ly.norm2))])
    return out + _named([("dec", tracker.decoder)])


def policy_tensors(actor, critic=None):
    """trunk W b per layer | mu W b | sigma W b or sigma_param | with a critic: critic W b.  The trunk (the shared Net) comes first."""
    from tianshou.utils.net.continuous import ActorProb
    if not isinstance(actor, ActorProb):
        raise ActorKindError("the device VirtualTaobao rollout and learner='device' need a continuous ActorProb actor "
                             "(Independent(Normal) policy)")
    if critic is not None and critic.preprocess is not actor.preprocess:
        raise ValueError("learner='device' needs actor and critic over one shared Net trunk (CIRS-RL-taobao.py)")
    trunk = linears(actor.preprocess.model, "actor trunk")
    heads = [("mu", actor.mu)] + ([("sigma", actor.sigma)] if actor._c_sigma else []) + ([("critic", critic.last)] if critic is not None else [])
    heads = [(k, linears(mlp, f"{k} head")) for k, mlp in heads]
    if any(len(lin) != 1 for _, lin in heads):
        raise ValueError("ActorProb / Critic heads with hidden layers are not supported by the device rollout and learner "
                         "(hidden_sizes=() only)")
    if int(actor.output_dim) != ACTION_DIM:
        raise ValueError(f"the actor must output the {ACTION_DIM} VirtualTaobao action features")
    if not 1 <= len(trunk) <= abi.VTB_RO_MAX_HIDDEN or any(m.out_features > 128 for m in trunk) or trunk[0].in_features > 128:
        raise ValueError("the trunk must be a Net of 1..3 hidden layers of width <= 128")
    out = _named([(f"trunk{i}", m) for i, m in enumerate(trunk)] + [(k, lin[0]) for k, lin in heads])
    if not actor._c_sigma:      # the free parameter sits where the sigma head would: after mu, before the critic
        out.insert(2 * len(trunk) + 2, ("sigma_param", actor.sigma_param))
    return out


class VtbModel:
    """`tracker` a HostStateTracker, `actor` an ActorProb over a Net trunk, `critic` (the learner's) the Critic over the same Net."""

    def __init__(self, tracker, actor, critic=None):
        self.tracker, self.actor = tracker, actor
        self._tensors = tracker_tensors(tracker), policy_tensors(actor, critic)
        trunk = linears(actor.preprocess.model, "actor trunk")
        self.hidden = [int(m.out_features) for m in trunk]
        if trunk[0].in_features != int(tracker.dim_state):
            raise ValueError("the actor trunk must be a Net of 1..3 hidden layers over the tracker state")

    def tracker_tensors(self):
        return list(self._tensors[0])

    def policy_tensors(self):
        return list(self._tensors[1])

    @property
    def dropout_p(self):
        """nn.Dropout is live while the tracker is in training mode (the reference never switches it off)."""
        return float(self.tracker.pos_encoder.dropout.p) if self.tracker.training else 0.0

    def model_cfg(self):
        """cirs_vtb_model_cfg of the modules; the dropout key (dropout_p, drop_env_base, dropout_seed) is per collect and left 0."""
        tracker, actor, n = self.tracker, self.actor, len(self.hidden)
        layers = tracker.transformer_encoder.layers
        return abi.VtbModelCfg(dim_model=int(tracker.dim_model), nhead=int(layers[0].self_attn.num_heads),
                               d_hid=int(layers[0].linear1.out_features), nlayers=len(layers), dim_state=int(tracker.dim_state),
                               max_len=int(tracker.MAX_TURN), n_hidden=n, max_action=float(actor._max),
                               hidden=(C.c_int32 * abi.VTB_RO_MAX_HIDDEN)(*self.hidden + [0] * (abi.VTB_RO_MAX_HIDDEN - n)),
                               unbounded=int(bool(actor._unbounded)), conditioned_sigma=int(bool(actor._c_sigma)))
