"""The six slot trackers' entry points as the library exports them, called without a GPU: every call here returns from the host-side checks
before anything is launched.  Shared by tools/gen_golden_slot_workspace.py (records) and test_slot_library_cpu.py (compares)."""
import ctypes as C
import itertools

from cirs_hip import abi

# tracker -> (cfg struct, weights / grads struct, state struct, the cfg's own fields in the variants the golden file covers)
TRACKERS = {
    "gru": (abi.GruCfg, abi.GruWeights, abi.GruState, [dict(nlayers=1), dict(nlayers=2)]),
    "lstm": (abi.LstmCfg, abi.LstmWeights, abi.LstmState, [dict(nlayers=1), dict(nlayers=2)]),
    "avg": (abi.AvgCfg, abi.AvgWeights, abi.AvgState, [dict(window=1), dict(window=10)]),
    "caser": (abi.CaserCfg, abi.CaserWeights, abi.CaserState,
              [dict(window=10, n_heights=3, heights=[2, 3, 4, 0]), dict(window=1, n_heights=1, heights=[1, 0, 0, 0])]),
    "nextitnet": (abi.NextItNetCfg, abi.NextItNetWeights, abi.NextItNetState,
                  [dict(n_blocks=1, dilations=[1, 0, 0, 0]), dict(n_blocks=3, dilations=[1, 2, 4, 0]), dict(n_blocks=4, dilations=[1, 1, 1, 4])]),
    "stamp": (abi.StampCfg, abi.StampWeights, abi.StampState, [dict(window=1), dict(window=16)]),
}
N_ROWS = [1, 63, 64, 65, 16384, 16385]      # the slab count's floor, its step at 64 rows, its cap of 256 slabs
N_ENVS = [1, 100]
DIM_STATES = [1, 20, 32]
# one common field made bad in an otherwise valid cfg; then several at once, with and without a fault in the tracker's own fields (OWN_BAD): the order of reports
BAD_FIELDS = [dict(dim_model=16), dict(dim_state=0), dict(dim_state=33), dict(max_len=0), dict(max_len=4097), dict(n_env=0),
              dict(dim_model=16, dim_state=0, max_len=0, n_env=0), dict(dim_state=0, max_len=0, n_env=0), dict(max_len=0, n_env=0),
              dict(own=True, dim_model=16, dim_state=0, max_len=0, n_env=0), dict(own=True, dim_state=0, max_len=0, n_env=0), dict(own=True)]
OWN_BAD = {"gru": dict(nlayers=3), "lstm": dict(nlayers=0), "avg": dict(window=0), "caser": dict(n_heights=5), "nextitnet": dict(n_blocks=0),
           "stamp": dict(window=17)}
REFUSED_N_ROWS = 7


def cfg_fields(name, variant=0, **over):
    f = dict(n_users=50, n_items=80, dim_model=32, dim_state=20, max_len=12, n_env=4)
    f.update(TRACKERS[name][3][variant])
    if over.pop("own", False):
        f.update(OWN_BAD[name])
    f.update(over)
    return f


def workspace_cfgs(name):
    for v, b, s in itertools.product(range(len(TRACKERS[name][3])), N_ENVS, DIM_STATES):
        yield cfg_fields(name, v, n_env=b, dim_state=s)


def make_cfg(name, fields):
    cls = TRACKERS[name][0]
    types = dict(cls._fields_)
    return cls(**{k: (types[k](*v) if isinstance(v, list) else v) for k, v in fields.items()})


_HOST = C.create_string_buffer(64)
DUMMY = (C.addressof(_HOST) + 15) & ~15      # a 16-byte aligned non-null address; nothing called here reads through it


def filled(cls, value=DUMMY):
    """An instance of a pointer-only struct with every pointer (nested structs and arrays included) set to `value`."""
    def fill(obj):
        for k, t in obj._fields_:
            if t is C.c_void_p:
                setattr(obj, k, value)
            elif issubclass(t, C.Array) and t._type_ is C.c_void_p:
                setattr(obj, k, t(*([value] * t._length_)))
            elif issubclass(t, C.Array):
                for item in getattr(obj, k):
                    fill(item)
            else:
                raise TypeError(f"{cls.__name__}.{k}: not a pointer")
    obj = cls()
    fill(obj)
    return obj


def _fn(lib, name, what):
    return getattr(lib, f"cirs_{name}_tracker_{what}")


def workspace_bytes(lib, name, cfg, n_rows):
    return int(_fn(lib, name, "backward_workspace_bytes")(None if cfg is None else C.byref(cfg), n_rows))


def _result(lib, rc):
    return [int(rc), lib.cirs_last_error().decode() if rc != 0 else ""]


def three_calls(lib, name, cfg, w):
    """init, step and backward with every other pointer null: [[rc, message], ...] in that order."""
    ref = C.byref(cfg)
    return [_result(lib, _fn(lib, name, "init")(ref, w, None, None, None, 2, None, 20, None)),
            _result(lib, _fn(lib, name, "step")(ref, w, None, None, None, None, None, 2, None, 20, None)),
            _result(lib, _fn(lib, name, "backward")(ref, w, None, None, None, None, None, None, None, None, 4, None, None, None, 0, None))]


def refused_calls(lib, name, cfg):
    """The three calls with null weights (as the trackers' own CPU tests call them) and with a weights struct of null pointers."""
    return {"null": three_calls(lib, name, cfg, None), "zeroed": three_calls(lib, name, cfg, C.byref(TRACKERS[name][1]()))}


def entry_sequence(lib, name, cfg):
    """A valid cfg walked through the checks of init, step and the head of backward one refusal at a time: [[label, rc, message], ...].
    Every call returns before a launch: the last check each one reaches fails (or n = 0 returns at once)."""
    _, wcls, scls, _ = TRACKERS[name]
    ref, S = C.byref(cfg), cfg.dim_state
    w, zw, st = C.byref(filled(wcls)), C.byref(wcls()), C.byref(filled(scls))
    init, step, bwd = _fn(lib, name, "init"), _fn(lib, name, "step"), _fn(lib, name, "backward")
    P = DUMMY
    need = workspace_bytes(lib, name, cfg, 4)
    out = []

    def rec(label, rc):
        out.append([label] + _result(lib, rc))
    rec("init weights null", init(ref, None, st, P, None, 2, P, S, None))
    rec("init weight pointers null", init(ref, zw, st, P, None, 2, P, S, None))
    rec("init n = 0", init(ref, w, None, None, None, 0, None, 0, None))
    rec("init users null", init(ref, w, st, None, None, 2, P, S, None))
    rec("init stride", init(ref, w, st, P, None, 2, P, S - 1, None))
    rec("init state null", init(ref, w, None, P, None, 2, P, S, None))
    rec("step weights null", step(ref, None, st, P, P, None, None, 2, P, S, None))
    rec("step weight pointers null", step(ref, zw, st, P, P, None, None, 2, P, S, None))
    rec("step n = 0", step(ref, w, None, None, None, None, None, 0, None, 0, None))
    rec("step rew null", step(ref, w, st, P, None, None, None, 2, P, S, None))
    rec("step stride", step(ref, w, st, P, P, None, None, 2, P, S - 1, None))
    rec("step state null", step(ref, w, None, P, P, None, None, 2, P, S, None))

    def backward(w_=w, st_=st, lens=P, n_rows=4, grads=w, ws=P, ws_bytes=need):
        return bwd(ref, w_, st_, P, P, P, P, P, P, lens, n_rows, P, grads, ws, ws_bytes, None)
    rec("backward weights null", backward(w_=None))
    rec("backward weight pointers null", backward(w_=zw))
    rec("backward lens null", backward(lens=None, n_rows=0, grads=zw, ws_bytes=0))      # the first of several faults is the one reported
    rec("backward n_rows = 0", backward(n_rows=0, grads=zw, ws_bytes=0))
    rec("backward gradient pointers null", backward(grads=zw, n_rows=1 << 27, ws_bytes=0))
    rec("backward n_rows out of range", backward(n_rows=1 << 27, ws_bytes=0))           # the trackers without a range check: workspace too small
    rec("backward workspace too small", backward(ws_bytes=need - 1, ws=P + 4))
    rec("backward workspace misaligned", backward(ws=P + 4))
    return out
