"""CPU: cirs_hip/vtb_model.py, the one description of the VirtualTaobao tracker + actor that the device rollout and the device learner
share: tensor order (the learner's images, the rollout's [in][out] image derived from the same lists), the geometry of
cirs_vtb_model_cfg and every refusal.  No GPU and no library needed."""
import types

import numpy as np
import pytest
import torch

import vtbrolloutcase as case


def _stack(hidden=(64, 64), dim_state=20, conditioned_sigma=False, mu_hidden=(), out_dim=27, own_critic_net=False, max_turn=50):
    """The script shape (max_turn 50, D 27, 3 heads, d_hid 128, 2 layers, Net (64, 64)) with distinct random values in every tensor."""
    from gym import spaces
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ActorProb, Critic
    space = spaces.Box(low=-1.0, high=1.0, shape=(27,), dtype=np.float32)
    tracker, actor, critic, policy = case.stack(types.SimpleNamespace(action_space=space), 4, max_turn, dim_state=dim_state, hidden=hidden)
    if conditioned_sigma or mu_hidden or out_dim != 27:
        actor = ActorProb(actor.preprocess, (out_dim,), hidden_sizes=mu_hidden, max_action=1.0, device="cpu", conditioned_sigma=conditioned_sigma)
    if own_critic_net:
        critic = Critic(Net(dim_state, hidden_sizes=list(hidden), device="cpu"), device="cpu")
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in list(tracker.parameters()) + list(actor.parameters()) + list(critic.parameters()):
            p.copy_(torch.randn(p.shape, generator=g))
    return tracker, actor, critic, policy


def test_tensor_lists_are_the_learner_images_in_make_layout_order():
    from cirs_hip.vtb_learn import pack_image, policy_params, tracker_params
    from cirs_hip.vtb_model import VtbModel
    tracker, actor, critic, policy = _stack()
    model = VtbModel(tracker, actor, critic)
    tt, pt = model.tracker_tensors(), model.policy_tensors()
    # make_layout (csrc/vtb_learn.hip): TLay then PLay, by name
    layer = ["in_w", "in_b", "out_w", "out_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b"]
    assert [n for n, _ in tt] == ["user_w", "user_b", "gate_w", "gate_b"] + [f"layer{l}.{k}" for l in range(2) for k in layer] + ["dec_w", "dec_b"]
    assert [n for n, _ in pt] == ["trunk0_w", "trunk0_b", "trunk1_w", "trunk1_b", "mu_w", "mu_b", "sigma_param", "critic_w", "critic_b"]
    assert [tuple(p.shape) for _, p in tt[:6]] == [(27, 88), (27,), (27, 28), (27,), (81, 27), (81,)]
    assert {id(p) for _, p in tt} == {id(p) for p in tracker.parameters()} and len(tt) == len(list(tracker.parameters()))
    assert {id(p) for _, p in pt} == {id(p) for p in list(actor.parameters()) + list(critic.parameters())}
    # (a) the concatenation of the lists is what pack_image packs
    opt_p, opt_t = policy.optim
    for tensors, params, opt in ((pt, policy_params(actor, critic), opt_p), (tt, tracker_params(tracker), opt_t)):
        assert all(a is b for (_, a), b in zip(tensors, params)) and len(tensors) == len(params)
        flat = pack_image(params, opt)[0]
        assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for _, p in tensors]))
    # conditioned sigma: the head takes sigma_param's place
    _, actor_c, critic_c, _ = _stack(conditioned_sigma=True)
    assert [n for n, _ in VtbModel(tracker, actor_c, critic_c).policy_tensors()][4:] == ["mu_w", "mu_b", "sigma_w", "sigma_b", "critic_w", "critic_b"]


def test_rollout_image_is_derived_from_the_same_lists():
    from cirs_hip.vtb_model import VtbModel
    from cirs_hip.vtb_rollout import fill_image, image_parts
    tracker, actor, critic, policy = _stack()
    assert policy.action_scaling
    model = VtbModel(tracker, actor, critic)      # with the critic: its tensors must not reach the rollout's image
    parts, total = image_parts(model, policy)
    slices = [(o, p.numel()) for _, p, _, o in parts]
    host = torch.full((total,), float("nan"))
    fill_image(host, parts)
    named = dict(model.tracker_tensors() + model.policy_tensors())
    names = [n for n, _, _, _ in parts]
    order = [n for n in named if not n.startswith("critic")]
    assert names == order[:4] + ["pe"] + order[4:] + ["act_low", "act_high"]      # cirs_vtb_policy_weights' own order
    end = 0
    for (name, _, _, _), (o, n) in zip(parts, slices):
        assert o % 4 == 0 and o == (end + 3) // 4 * 4, name      # 16-byte aligned, packed
        got = host[o:o + n]
        if name in named:      # (b) a matrix transposed ([out][in] -> [in][out]), a vector flat
            p = named[name].detach()
            assert n == p.numel() and torch.equal(got, (p.t() if p.dim() == 2 else p).reshape(-1)), name
        end = o + n
    at = dict(zip(names, slices))
    o, n = at["pe"]
    assert torch.equal(host[o:o + n], tracker.pos_encoder.pe[:, 0, :].reshape(-1)) and n == tracker.MAX_TURN * 27
    for name, bound in (("act_low", policy.action_space.low), ("act_high", policy.action_space.high)):
        o, n = at[name]
        assert n == 27 and np.array_equal(host[o:o + n].numpy(), np.asarray(bound, np.float32))
    assert total == (end + 3) // 4 * 4 and int(torch.isnan(host).sum()) == total - sum(n for _, n in slices)      # only the alignment gaps stay unwritten
    # a later change of the host parameters reaches the next image (the rollout packs before every collect)
    with torch.no_grad():
        actor.mu.model[0].weight.add_(1.0)
    fill_image(host, parts)
    o, n = at["mu_w"]
    assert torch.equal(host[o:o + n], actor.mu.model[0].weight.detach().t().reshape(-1))


def test_model_cfg_reads_the_geometry_once():
    from cirs_hip.vtb_model import VtbModel
    tracker, actor, critic, _ = _stack(hidden=(64, 32))
    m = VtbModel(tracker, actor, critic).model_cfg()
    assert (m.dim_model, m.nhead, m.d_hid, m.nlayers, m.dim_state, m.max_len) == (27, 3, 128, 2, 20, tracker.MAX_TURN)
    assert m.max_len >= 50 + 1      # positions 0..max_turn
    assert (m.n_hidden, list(m.hidden), m.unbounded, m.conditioned_sigma, m.max_action) == (2, [64, 32, 0], 0, 0, 1.0)
    assert (m.dropout_p, m.drop_env_base, m.dropout_seed) == (0.0, 0, 0)      # the key of a collect is not the model's


def test_dropout_is_live_only_in_training_mode():
    from cirs_hip.vtb_model import VtbModel
    tracker, actor, _, _ = _stack()
    tracker.pos_encoder.dropout.p = 0.1
    model = VtbModel(tracker, actor)
    tracker.train()
    assert model.dropout_p == pytest.approx(0.1)
    tracker.eval()
    assert model.dropout_p == 0.0


@pytest.mark.parametrize("kw,match", [
    (dict(mu_hidden=(16,)), "hidden layers"),
    (dict(conditioned_sigma=True, mu_hidden=(16,)), "hidden layers"),
    (dict(out_dim=26), "27 VirtualTaobao action features"),
    (dict(hidden=()), "1..3 hidden layers"),
    (dict(hidden=(16, 16, 16, 16)), "1..3 hidden layers"),
    (dict(hidden=(129,)), "width <= 128"),
    (dict(own_critic_net=True), "shared Net trunk"),
])
def test_refusals(kw, match):
    from cirs_hip.vtb_learn import policy_params
    from cirs_hip.vtb_model import VtbModel
    tracker, actor, critic, _ = _stack(**kw)
    with pytest.raises(ValueError, match=match):
        VtbModel(tracker, actor, critic)
    with pytest.raises(ValueError, match=match):
        policy_params(actor, critic)
    if "own_critic_net" not in kw:      # the rollout's model has no critic
        with pytest.raises(ValueError, match=match):
            VtbModel(tracker, actor)


def test_a_trunk_over_another_width_than_the_tracker_state_is_refused():
    from cirs_hip.vtb_model import VtbModel
    tracker, _, _, _ = _stack(dim_state=20)
    _, actor, critic, _ = _stack(dim_state=24)
    with pytest.raises(ValueError, match="over the tracker state"):
        VtbModel(tracker, actor, critic)


def test_an_actor_of_another_class_is_a_type_error_and_a_value_error():
    """DeviceVtbRollout has raised TypeError for it, policy_params ValueError: both stay catchable."""
    from cirs_hip.vtb_learn import policy_params
    from cirs_hip.vtb_model import VtbModel
    from tianshou.utils.net.discrete import Actor
    tracker, actor, critic, _ = _stack()
    other = Actor(actor.preprocess, 27, device="cpu")
    for kind in (TypeError, ValueError):
        with pytest.raises(kind, match="ActorProb"):
            VtbModel(tracker, other)
        with pytest.raises(kind, match="ActorProb"):
            policy_params(other, critic)


@pytest.mark.parametrize("break_it,match", [
    (lambda tr: setattr(tr.transformer_encoder.layers[1], "norm_first", True), "post-norm ReLU"),
    (lambda tr: setattr(tr.transformer_encoder.layers[0], "activation", torch.nn.functional.gelu), "post-norm ReLU"),
    (lambda tr: setattr(tr.decoder, "bias", None), "needs a bias"),
])
def test_tracker_refusals(break_it, match):
    from cirs_hip.vtb_learn import tracker_params
    from cirs_hip.vtb_model import VtbModel
    tracker, actor, critic, _ = _stack()
    break_it(tracker)
    with pytest.raises(ValueError, match=match):
        VtbModel(tracker, actor, critic)
    with pytest.raises(ValueError, match=match):
        tracker_params(tracker)


def test_a_layer_that_is_neither_linear_nor_relu_is_refused():
    from cirs_hip.vtb_model import VtbModel, linears
    tracker, actor, critic, _ = _stack()
    assert len(linears(actor.preprocess.model, "actor trunk")) == 2
    actor.preprocess.model.model[1] = torch.nn.Tanh()
    with pytest.raises(ValueError, match="actor trunk: only Linear \\+ ReLU.*Tanh"):
        VtbModel(tracker, actor, critic)
