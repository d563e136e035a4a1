"""CPU: the one filler of the nine slot trackers' weight structs (cirs_hip/slot_engine.py: fill_weights over an engine's FIELDS table) puts every
tensor's address into the member its table names and leaves the indexed members beyond the live count null; the table reaches every tensor of
the tracker's x_param_shapes; a tensor of another shape (the same element count included), dtype or layout and a missing tensor are refused
by name -- by the filler and by each DeviceXTracker constructor, there before the library is loaded or a device tensor is allocated.  The
kernels index these pointers by the cfg's sizes alone, so on a device the refusals are what stands between a wrong tensor and a read out of
bounds.  No GPU and no library call."""
import importlib
import re

import pytest
import torch

from cirs_hip import abi, slot_engine
from cirs_hip.slot_engine import DECODER_FIELDS, HEAD_FIELDS, DeviceSlotTracker, fill_weights

U, I, S, B, T = 5, 7, 20, 3, 20
GATE = "fnn_gate.weight"
# tracker, engine class, the model as x_param_shapes takes it, what the constructor takes besides, live indices, a tensor of its own and which of
# its dimensions the refusal test moves by one: the smallest and the largest model of every tracker, so both ends of every indexed member
VARIANTS = [
    ("gru", "DeviceGruTracker", dict(nlayers=1), {}, 1, ("gru.weight_hh_l0", 0)),
    ("gru", "DeviceGruTracker", dict(nlayers=2), {}, 2, ("gru.bias_ih_l1", 0)),
    ("lstm", "DeviceLstmTracker", dict(nlayers=1), {}, 1, ("lstm.weight_ih_l0", 1)),
    ("lstm", "DeviceLstmTracker", dict(nlayers=2), {}, 2, ("lstm.bias_hh_l1", 0)),
    ("avg", "DeviceAvgTracker", {}, dict(window_size=3), 0, None),
    ("caser", "DeviceCaserTracker", dict(window_size=1, filter_sizes=(1,)), {}, 1, ("horizontal_cnn.0.weight", 2)),
    ("caser", "DeviceCaserTracker", dict(window_size=16, filter_sizes=(1, 2, 3, 4)), {}, 4, ("vertical_cnn.weight", 2)),      # built for window 17
    ("nextitnet", "DeviceNextItNetTracker", dict(dilations=(1,)), {}, 1, ("blocks.0.conv.weight", 2)),
    ("nextitnet", "DeviceNextItNetTracker", dict(dilations=(1, 2, 2, 2)), {}, 4, ("blocks.3.ln.bias", 0)),      # four blocks: the most the build has
    ("stamp", "DeviceStampTracker", {}, dict(window_size=1), 0, ("attn.w0.weight", 0)),
    ("stamp", "DeviceStampTracker", {}, dict(window_size=16), 0, ("mlp_b.weight", 1)),
    ("narm", "DeviceNarmTracker", {}, {}, 1, ("bilinear.weight", 1)),
    ("fmlp", "DeviceFmlpTracker", dict(window_size=1, nlayers=1), {}, 1, ("layers.0.filter.complex_weight", 0)),
    ("fmlp", "DeviceFmlpTracker", dict(window_size=16, nlayers=2), {}, 2, ("layers.1.filter.complex_weight", 0)),      # built for window 14
    ("lru", "DeviceLruTracker", {}, {}, 1, ("lru.in_proj.weight", 0)),
]
IDS = [f"{v[0]}-{'-'.join(str(x) for x in {**v[2], **v[3]}.values()) or 'plain'}".replace(" ", "") for v in VARIANTS]


@pytest.fixture(params=VARIANTS, ids=IDS)
def variant(request):
    name, engine, model, extra, live, own = request.param
    mod = importlib.import_module(f"cirs_hip.{name}_tracker")
    shapes = getattr(mod, f"{name}_param_shapes")(U, I, dim_state=S, **model)
    params = {k: torch.zeros(sh, dtype=torch.float32) for k, sh in shapes.items()}
    return getattr(mod, engine), shapes, params, {**model, **extra}, live, own


def _member(w, member, i):
    """The pointer a table's member spelling names: "m", "m[]" at i, "m[].f" at i."""
    array, indexed, sub = member.partition("[]")
    if not indexed:
        return getattr(w, member)
    elem = getattr(w, array)[i]
    return getattr(elem, sub[1:]) if sub else elem


def _bump(t, dim):
    shape = list(t.shape)
    shape[dim] += 1
    return torch.zeros(shape, dtype=t.dtype)


def _bad_tensors(params, own):
    """(name, a tensor the filler must refuse under that name): the gate matrix transposed in shape only -- the same 1056 elements, contiguous,
    so nothing but a shape check sees it -- then one of the tracker's own tensors with one dimension off by one, a float64 and a strided view."""
    bad = [(GATE, torch.zeros((33, 32))), ("decoder.bias", params["decoder.bias"].double()), ("ffn_user.weight", params["ffn_user.weight"].t())]
    if own is not None:
        bad.append((own[0], _bump(params[own[0]], own[1])))
        strided = _bump(params[own[0]], -1)[..., :-1]      # the right shape, not contiguous
        if not strided.is_contiguous():
            bad.append((own[0], strided))
    return bad


def test_the_table_spells_the_struct_and_reaches_every_tensor(variant):
    engine, shapes, params, kw, live, own = variant
    assert [m for m, _ in HEAD_FIELDS + list(engine.FIELDS) + DECODER_FIELDS] == slot_engine.struct_members(engine.WEIGHTS)
    w = fill_weights(engine.WEIGHTS, engine.FIELDS, live, shapes, params)
    named = set()
    for member, name in HEAD_FIELDS + list(engine.FIELDS) + DECODER_FIELDS:
        if "[]" not in member:
            assert "{}" not in name and _member(w, member, None) == params[name].data_ptr(), name
            named.add(name)
            continue
        size = len(getattr(w, member.partition("[]")[0]))
        assert "{}" in name and live <= size
        for i in range(size):
            if i < live:
                assert _member(w, member, i) == params[name.format(i)].data_ptr(), name.format(i)
                named.add(name.format(i))
            else:
                assert not _member(w, member, i), (member, i)      # beyond the live count: null
    assert named == set(shapes)      # no tensor of the tracker is left out of the struct
    assert len({t.data_ptr() for t in params.values()}) == len(params)      # the addresses tell the tensors apart


def test_fmlp_filter_shapes_at_the_window_ends():
    from cirs_hip.fmlp_tracker import fmlp_param_shapes
    assert fmlp_param_shapes(U, I, 32, S, 1, 1)["layers.0.filter.complex_weight"] == (1, 32, 2)
    assert fmlp_param_shapes(U, I, 32, S, 16, 2)["layers.1.filter.complex_weight"] == (9, 32, 2)


def test_the_filler_refuses_by_name(variant):
    engine, shapes, params, kw, live, own = variant
    for name, t in _bad_tensors(params, own):
        with pytest.raises(ValueError, match=re.escape(name)) as e:
            fill_weights(engine.WEIGHTS, engine.FIELDS, live, shapes, {**params, name: t})
        if t.dtype == torch.float32 and t.is_contiguous():      # a shape refusal gives both shapes
            assert str(tuple(t.shape)) in str(e.value) and str(tuple(shapes[name])) in str(e.value)
    for name in (GATE, "decoder.weight") + (() if own is None else (own[0],)):
        with pytest.raises(KeyError, match=re.escape(name)):
            fill_weights(engine.WEIGHTS, engine.FIELDS, live, shapes, {k: v for k, v in params.items() if k != name})


def test_every_engine_constructor_refuses_before_the_device(variant, monkeypatch):
    engine, shapes, params, kw, live, own = variant
    bad = _bad_tensors(params, own)      # built before torch.zeros is taken away

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library or the device")
    monkeypatch.setattr(abi, "lib", no_device)
    monkeypatch.setattr(torch, "zeros", no_device)
    assert issubclass(engine, DeviceSlotTracker) and "_weights" not in vars(engine)
    for name, t in bad:
        with pytest.raises(ValueError, match=re.escape(name)):
            engine({**params, name: t}, U, I, B, T, dim_state=S, **kw)
    with pytest.raises(KeyError, match=re.escape(GATE)):
        engine({k: v for k, v in params.items() if k != GATE}, U, I, B, T, dim_state=S, **kw)
    with pytest.raises(AssertionError, match="touched"):      # the right tensors pass the filler and reach the first allocation
        engine(params, U, I, B, T, dim_state=S, **kw)
    with pytest.raises(TypeError):
        engine(params, U, I, B, T, dim_state=S, no_such_keyword=1, **kw)


def test_a_table_that_does_not_spell_its_struct_is_refused_at_class_creation():
    from cirs_hip.stamp_tracker import DeviceStampTracker
    for fields in (DeviceStampTracker.FIELDS[:-1], DeviceStampTracker.FIELDS[1:] + DeviceStampTracker.FIELDS[:1], [("w1[]", "attn.w{}.weight")]):
        with pytest.raises(TypeError, match="FIELDS"):
            type("Broken", (DeviceStampTracker,), {"FIELDS": fields})
