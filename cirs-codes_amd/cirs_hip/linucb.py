"""The disjoint-arm LinUCB bandit on the device (csrc/linucb.hip: cirs_linucb_update / _solve / _score / _predict).

Counterpart of reference core/policy/linucb.py: K arms, each with A [d, d] = I + sum x x^T and b [d] = sum reward x in float64.
DeviceLinUCB keeps A, b and the solved pair (A_inv, theta) resident; update() does the torch plumbing (stable sort of the rows by arm,
segment offsets) around the ordered accumulation kernel, solve() runs lazily for the arms an update touched, score() / score_x() /
predict() read the solved pair.  core/policy/linucb.py wraps it in the reference's class names."""
import numpy as np
import torch

from . import abi


def arm_of_rows(classes, raw_ids):
    """Position of every raw id in the sorted `classes` [K] (LabelEncoder.classes_), -1 where it is absent; int64 tensors, one device."""
    if classes.numel() == 0:
        return torch.full_like(raw_ids, -1)
    pos = torch.searchsorted(classes, raw_ids).clamp_(max=classes.numel() - 1)
    return torch.where(classes[pos] == raw_ids, pos, torch.full_like(pos, -1))


class DeviceLinUCB:
    def __init__(self, K, d, alpha, device="cuda"):
        if not 2 <= int(d) <= 16:
            raise ValueError("LinUCB on the device: d must lie in [2, 16]")
        self.K, self.d, self.alpha = int(K), int(d), float(alpha)
        self.device = torch.device(device)
        eye = torch.eye(self.d, dtype=torch.float64, device=self.device)
        self.A = eye.repeat(self.K, 1, 1).contiguous()
        self.b = torch.zeros((self.K, self.d), dtype=torch.float64, device=self.device)
        self._A_inv = eye.repeat(self.K, 1, 1).contiguous()
        self._theta = torch.zeros((self.K, self.d), dtype=torch.float64, device=self.device)
        self._dirty_all = False          # an update touched any number of arms
        self._dirty = set()              # or these arms alone (one-row updates)
        self._lib = abi.lib()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _f64(self, t):
        return torch.as_tensor(np.asarray(t, np.float64) if not isinstance(t, torch.Tensor) else t).to(self.device, torch.float64)

    # ---- accumulation --------------------------------------------------------------------------------------------------------------
    def plan(self, arm_of_row):
        """(order [m], seg [K + 1]) of a log: the rows with an arm grouped by arm, in log order inside an arm."""
        arm = torch.as_tensor(arm_of_row).to(self.device, torch.int64)
        rows = torch.nonzero(arm >= 0).reshape(-1)
        arms_sorted, perm = torch.sort(arm[rows], stable=True)
        seg = torch.zeros(self.K + 1, dtype=torch.int64, device=self.device)
        seg[1:] = torch.cumsum(torch.bincount(arms_sorted, minlength=self.K), 0)
        return rows[perm].contiguous(), seg

    def update(self, x, y, arm_of_row=None, plan=None):
        """Add the rows x [n, >= d], y [n] of a log: row r goes to arm arm_of_row[r] (-1: to none).  `plan`: the result of plan() for the
        same arm_of_row, to reuse it over epochs."""
        x = self._f64(x)
        if x.dim() != 2 or x.shape[1] < self.d or x.stride(1) != 1:
            x = x.reshape(-1, x.shape[-1]).contiguous()
        y = self._f64(y).reshape(-1).contiguous()
        assert x.shape[1] >= self.d and y.numel() == x.shape[0], "x [n, >= d] and y [n] must have one row per sample"
        order, seg = plan if plan is not None else self.plan(arm_of_row)
        abi.check(self._lib.cirs_linucb_update(self.A.data_ptr(), self.b.data_ptr(), self.K, self.d, x.data_ptr(), x.stride(0), x.shape[0],
                                               y.data_ptr(), order.data_ptr(), order.numel(), seg.data_ptr(), self._stream()), "cirs_linucb_update")
        if order.numel():
            self._dirty_all = True

    def update_one(self, arm, reward, x):
        """reward_update of one arm with one row."""
        x = self._f64(x).reshape(1, -1).contiguous()
        y = torch.full((1,), float(np.asarray(reward, np.float64).reshape(-1)[0]), dtype=torch.float64, device=self.device)
        order = torch.zeros(1, dtype=torch.int64, device=self.device)
        seg = torch.zeros(self.K + 1, dtype=torch.int64, device=self.device)
        seg[int(arm) + 1:] = 1
        abi.check(self._lib.cirs_linucb_update(self.A.data_ptr(), self.b.data_ptr(), self.K, self.d, x.data_ptr(), x.stride(0), 1, y.data_ptr(),
                                               order.data_ptr(), 1, seg.data_ptr(), self._stream()), "cirs_linucb_update")
        self._dirty.add(int(arm))

    # ---- solve (lazy) --------------------------------------------------------------------------------------------------------------
    def solve(self):
        """(A_inv [K, d, d], theta [K, d]) of the current A, b; runs only for what an update touched since the last call."""
        if self._dirty_all or self._dirty:
            arms = None if self._dirty_all else torch.as_tensor(sorted(self._dirty), dtype=torch.int32).to(self.device)
            abi.check(self._lib.cirs_linucb_solve(self.A.data_ptr(), self.b.data_ptr(), self.K, self.d, abi.ptr(arms),
                                                  0 if arms is None else arms.numel(), self._A_inv.data_ptr(), self._theta.data_ptr(),
                                                  self._stream()), "cirs_linucb_solve")
            self._dirty_all = False
            self._dirty.clear()
        return self._A_inv, self._theta

    @property
    def A_inv(self):
        return self.solve()[0]

    @property
    def theta(self):
        return self.solve()[1]

    # ---- readers -------------------------------------------------------------------------------------------------------------------
    def _score(self, users, item_feats, x_fixed, rows, want_full):
        A_inv, theta = self.solve()
        best = torch.full((rows,), -1, dtype=torch.int64, device=self.device)
        best_mean = torch.zeros(rows, dtype=torch.float64, device=self.device)
        ucb = torch.empty((rows, self.K), dtype=torch.float64, device=self.device) if want_full else None
        mean = torch.empty((rows, self.K), dtype=torch.float64, device=self.device) if want_full else None
        var = torch.empty((rows, self.K), dtype=torch.float64, device=self.device) if want_full else None
        abi.check(self._lib.cirs_linucb_score(A_inv.data_ptr(), theta.data_ptr(), self.K, self.d, abi.ptr(users), rows, abi.ptr(item_feats),
                                              abi.ptr(x_fixed), self.alpha, best.data_ptr(), best_mean.data_ptr(), abi.ptr(ucb), abi.ptr(mean),
                                              abi.ptr(var), self._stream()), "cirs_linucb_score")
        return (best, best_mean, ucb, mean, var) if want_full else (best, best_mean)

    def score(self, users, item_feats, want_full=False):
        """users [B] (raw ids), item_feats [K, d - 2] -> (first arg-max arm of the ucb [B] int64, that arm's mean [B]); want_full adds
        ucb, mean and var [B, K] each.  Arm a is scored at x = [user, a, item_feats[a]]."""
        users = self._f64(users).reshape(-1).contiguous()
        feats = self._f64(item_feats).reshape(self.K, self.d - 2).contiguous()
        return self._score(users, feats, None, users.numel(), want_full)

    def score_x(self, x):
        """One x [d] against every arm -> (ucb [K], mean [K])."""
        x = self._f64(x).reshape(-1).contiguous()
        assert x.numel() == self.d, "x must have d entries"
        _, _, ucb, mean, _ = self._score(None, None, x, 1, True)
        return ucb[0], mean[0]

    def predict(self, x, arm_of_row):
        """theta[arm_of_row[r]]^T x[r] for every row of x [n, >= d]; 0 where arm_of_row[r] is -1."""
        x = self._f64(x)
        if x.stride(1) != 1:
            x = x.contiguous()
        arm = torch.as_tensor(arm_of_row).to(self.device, torch.int64).contiguous()
        assert x.dim() == 2 and x.shape[1] >= self.d and arm.numel() == x.shape[0]
        _, theta = self.solve()
        out = torch.empty(x.shape[0], dtype=torch.float64, device=self.device)
        abi.check(self._lib.cirs_linucb_predict(theta.data_ptr(), self.K, self.d, x.data_ptr(), x.stride(0), arm.data_ptr(), x.shape[0],
                                                out.data_ptr(), self._stream()), "cirs_linucb_predict")
        return out
