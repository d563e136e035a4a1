"""The disjoint-arm LinUCB bandit restated in numpy float64 (reference core/policy/linucb.py), in a vectorised structure of its own.

What the four device operations of csrc/linucb.hip compute, for checking them: the CPU tests hold this file against the reference's
recorded results (tests/golden/linucb.npz), the GPU tests hold the device against it at shapes the fixture does not have.

  update   rows grouped by arm (stable), every arm adds its rows in log order: step r adds the r-th row of every arm that has one, so the
           sums of an arm are formed in the reference's order, one rounded product and one rounded sum per element and row -> A and b
           equal the reference's bit for bit
  solve    one batched np.linalg.inv, theta = inv(A) b
           (extended=True: a batched Cholesky solve with refinement in np.longdouble instead, and the scores in np.longdouble too,
           rounded to float64 at the end.  inv(A) is ill-conditioned here, cond_2 ~ 1e11, and the float64 solve above is wrong by
           about as much as the reference's own; the 64-bit significand brings that down 2048 times, which makes this mode the
           yardstick at shapes for which no exact values are recorded)
  score    x = [user, arm position, item features of the arm]: mean = theta^T x, ucb = mean + alpha sqrt(x^T inv(A) x), first arg-max
  predict  theta[arm]^T x per row, 0 for rows whose item is no arm"""
import numpy as np


def arm_of_rows(classes, raw_ids):
    """Position of every raw id in the sorted `classes` (LabelEncoder.classes_), -1 where it is absent."""
    classes = np.asarray(classes).astype(np.int64)
    ids = np.asarray(raw_ids).astype(np.int64)          # int(x[1]) of the reference: truncation
    if classes.size == 0:
        return np.full(ids.shape, -1, np.int64)
    pos = np.minimum(np.searchsorted(classes, ids), classes.size - 1)
    return np.where(classes[pos] == ids, pos, -1).astype(np.int64)


def group_rows(arm_of_row, K):
    """(order [m], seg [K + 1]): the rows with an arm, grouped by arm and in log order inside an arm; arm a owns order[seg[a]:seg[a + 1]]."""
    arm_of_row = np.asarray(arm_of_row, np.int64)
    rows = np.flatnonzero(arm_of_row >= 0)
    order = rows[np.argsort(arm_of_row[rows], kind="stable")]
    seg = np.concatenate([[0], np.cumsum(np.bincount(arm_of_row[rows], minlength=K))]).astype(np.int64)
    return order, seg


def tie_pick(ucb):
    """select_arm's choice among the arms of highest ucb (core/policy/linucb.py:77-103): the bound starts at -1; a new maximum resets the
    candidate list to that arm, which the tie test then appends once more; later arms equal to the maximum are appended once.  One draw
    of np.random.choice over that list."""
    ucb = np.asarray(ucb, np.float64).reshape(-1)
    candidates = []
    if ucb.size and ucb.max() > -1:
        first = int(np.argmax(ucb))
        candidates = [first, first] + [int(a) for a in np.flatnonzero(ucb == ucb[first]) if a > first]
    return np.random.choice(candidates)


class HostLinUCB:
    def __init__(self, K, d, alpha, extended=False):
        self.K, self.d, self.alpha = int(K), int(d), float(alpha)
        self.dtype = np.float64
        if extended:
            assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 on this platform"
            self.dtype = np.longdouble
        self.A = np.tile(np.identity(self.d), (self.K, 1, 1))
        self.b = np.zeros((self.K, self.d))
        self.A_inv = self.theta = None

    def update(self, x, y, arm_of_row):
        x = np.asarray(x, np.float64)[:, :self.d]
        y = np.asarray(y, np.float64).reshape(-1)
        order, seg = group_rows(arm_of_row, self.K)
        count = np.diff(seg)
        by_load = np.argsort(-count, kind="stable")         # arms by falling row count: the arms still active at step r are a prefix
        start, load = seg[:-1][by_load], count[by_load]
        for r in range(int(load[0]) if load.size else 0):
            live = int(np.searchsorted(-load, -r, side="left"))      # arms with more than r rows
            rows = order[start[:live] + r]
            arms = by_load[:live]
            xr = x[rows]
            self.A[arms] = self.A[arms] + xr[:, :, None] * xr[:, None, :]
            self.b[arms] = self.b[arms] + y[rows][:, None] * xr
        self.A_inv = self.theta = None

    def solve(self):
        if self.A_inv is None and self.dtype is np.float64:
            self.A_inv = np.linalg.inv(self.A) if self.K else np.zeros_like(self.A)
            self.theta = np.matmul(self.A_inv, self.b[:, :, None])[:, :, 0]
        elif self.A_inv is None:
            Z = self._solve_extended()
            self.A_inv, self.theta = Z[:, :, :self.d], Z[:, :, self.d]
        return self.A_inv, self.theta

    def _solve_extended(self):
        """A Z = [I | b] for every arm in np.longdouble: A = L L^T (A = I + sum x x^T is positive definite), two triangular solves,
        two refinement steps."""
        d = self.d
        A = self.A.astype(self.dtype)
        rhs = np.concatenate([np.tile(np.identity(d), (self.K, 1, 1)), self.b[:, :, None]], axis=2).astype(self.dtype)
        L = np.zeros_like(A)
        for i in range(d):
            for j in range(i + 1):
                v = A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)
                L[:, i, j] = np.sqrt(v) if i == j else v / L[:, j, j]

        def solve(R):
            Z = np.zeros_like(R)
            for i in range(d):
                Z[:, i] = (R[:, i] - (L[:, i, :i, None] * Z[:, :i]).sum(1)) / L[:, i, i, None]
            for i in reversed(range(d)):
                Z[:, i] = (Z[:, i] - (L[:, i + 1:, i, None] * Z[:, i + 1:]).sum(1)) / L[:, i, i, None]
            return Z
        Z = solve(rhs)
        for _ in range(2):
            Z = Z + solve(rhs - np.matmul(A, Z))
        return Z

    def arm_x(self, users, item_feats):
        users = np.asarray(users, np.float64).reshape(-1)
        feats = np.asarray(item_feats, np.float64).reshape(self.K, self.d - 2)
        x = np.empty((len(users), self.K, self.d))
        x[:, :, 0] = users[:, None]
        x[:, :, 1] = np.arange(self.K)[None, :]
        x[:, :, 2:] = feats[None]
        return x

    def score_x(self, x):
        """x [..., K, d] (or [d]: the same x for every arm) -> (ucb, mean, var) [..., K]."""
        A_inv, theta = self.solve()
        x = np.asarray(x, np.float64).astype(self.dtype)
        if x.ndim == 1:
            x = np.broadcast_to(x, (self.K, self.d))
        mean = np.einsum("...kd,kd->...k", x, theta)
        var = np.einsum("...kd,kde,...ke->...k", x, A_inv, x)
        ucb = mean + self.dtype(self.alpha) * np.sqrt(var)
        return ucb.astype(np.float64), mean.astype(np.float64), var.astype(np.float64)

    def score(self, users, item_feats):
        """-> (best arm [B], its mean [B], ucb [B, K], mean [B, K], var [B, K])."""
        ucb, mean, var = self.score_x(self.arm_x(users, item_feats))
        best = ucb.argmax(axis=1)
        return best, mean[np.arange(len(best)), best], ucb, mean, var

    def predict(self, x, arm_of_row):
        _, theta = self.solve()
        x = np.asarray(x, np.float64)[:, :self.d].astype(self.dtype)
        arm_of_row = np.asarray(arm_of_row, np.int64)
        hit = arm_of_row >= 0
        out = np.zeros(len(x))
        out[hit] = np.einsum("nd,nd->n", theta[arm_of_row[hit]], x[hit]).astype(np.float64)
        return out

    def select_arm(self, x):
        return tie_pick(self.score_x(np.asarray(x, np.float64).reshape(-1))[0])
