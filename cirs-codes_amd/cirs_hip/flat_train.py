"""What the device trainers share on the host side.

FlatTrainer    parameters, gradients and the Adam moments as ONE flat fp32 device buffer each, the step count, the workspace and the
               leading arguments of every _step / _epoch entry (mmoe_train.py: MMoETrainer, MlpTrainer; below: TableTrainer).
TableTrainer   the two Kuaishou trainers (deepfm_train.py, dice_train.py): named views over a layout list, a device-resident data set
               in column form and whole passes over it from one call of the model's _epoch entry."""
import ctypes as C

import numpy as np
import torch

from . import abi


class FlatTrainer:
    _workspace_bytes = None   # name of the ABI's workspace size query

    def _alloc(self, cfg, total, device):
        self.device = torch.device(device)
        self.cfg = cfg
        self._lib = abi.lib()
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros_like(self.flat)
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        self.step_count = 0
        self._ws = None

    def _workspace(self, n):
        """Grows, never shrinks."""
        need = getattr(self._lib, self._workspace_bytes)(C.byref(self.cfg), int(n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _buffers(self):
        return C.byref(self.cfg), self.flat.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.step_count


def fill_views(flat, layout, sd, absent):
    """{name: view of `flat`} along layout = [(state_dict name, shape)] in buffer order, each filled from sd; a name sd lacks takes the
    constant absent(name), which raises for a name that must be there."""
    views, off = {}, 0
    for name, shape in layout:
        n = int(np.prod(shape))
        views[name] = flat[off:off + n].view(shape)
        if name in sd:
            views[name].copy_(torch.as_tensor(sd[name]).to(flat.device, torch.float32).reshape(shape))
        else:
            views[name].fill_(absent(name))
        off += n
    assert off == flat.numel()
    return views


class TableTrainer(FlatTrainer):
    """A subclass names its ABI entries and loss columns, supplies split_columns(x, y, score, device) -> the device columns of its _epoch
    entry and _epoch_args() -> the entry's arguments between batch_size and losses_out, and may range-check a data set in _check_ids."""
    _param_count = _epoch_fn = None
    LOSS_COLUMNS = ()
    split_columns = None

    def _setup(self, cfg, layout, sd, absent, l2, lr, betas, eps, device):
        self._alloc(cfg, getattr(abi.lib(), self._param_count)(C.byref(cfg)), device)
        self.views = fill_views(self.flat, layout, sd, absent)
        self.l2 = tuple(float(c) for c in l2)                      # (l2_embedding, l2_linear, l2_all)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self._data = None
        self.loss = torch.zeros(len(self.LOSS_COLUMNS), dtype=torch.float32, device=self.device)

    def state_dict(self):
        return {k: v.clone() for k, v in self.views.items()}

    def _check_ids(self, cols):
        pass

    def _adam(self):
        return (*self.l2, self.lr, self.betas[0], self.betas[1], self.eps)

    def _run_epoch(self, cols, n_rows, order, n_order, batch_size):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if n_rows < 1 or n_order < 1:
            raise ValueError("empty data set or index array")
        steps = (n_order + batch_size - 1) // batch_size
        losses = torch.zeros(steps, len(self.LOSS_COLUMNS), dtype=torch.float32, device=self.device)
        ws = self._workspace(min(int(batch_size), n_order))
        abi.check(getattr(self._lib, self._epoch_fn)(*self._buffers(), *[c.data_ptr() for c in cols], n_rows, abi.ptr(order), n_order,
                                                     int(batch_size), *self._epoch_args(), losses.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     self._stream()), self._epoch_fn)
        self.step_count += steps
        return losses

    def _step_as_epoch(self, cols):
        """One optimiser step on a batch = a pass of one batch over these rows."""
        n = cols[0].numel()
        self.loss.copy_(self._run_epoch(cols, n, None, n, n)[0])
        return self.loss

    def load(self, x, y, score):
        """Make the data set resident on the device in the column form of the kernels (the split runs once); epoch() trains on it."""
        cols = type(self).split_columns(x, y, score, self.device)
        self._check_ids(cols)
        self._data = cols
        return cols[0].numel()

    def epoch(self, order, batch_size, check=True):
        """One pass over the loaded data set from one call: batch b is the rows order[b * batch_size : (b + 1) * batch_size] (int64 indices
        into the data set; None = every row in file order), the last batch short.  Returns the [steps, len(LOSS_COLUMNS)] device tensor of
        the per-step LOSS_COLUMNS.  check=False skips the range check of `order` (one read-back in front of the pass) for a caller that
        built the permutation itself; the kernel answers an index outside the data set with a NaN loss, not a read."""
        assert self._data is not None, "call load(x, y, score) first"
        n_rows = self._data[0].numel()
        if order is None:
            return self._run_epoch(self._data, n_rows, None, n_rows, batch_size)
        order = torch.as_tensor(order).to(self.device, torch.int64).reshape(-1).contiguous()
        if check and order.numel():
            lo, hi = torch.aminmax(order)     # checked in front of the pass; the steps themselves run without a host round trip
            if int(lo) < 0 or int(hi) >= n_rows:
                raise IndexError(f"order holds row indices outside [0, {n_rows})")
        return self._run_epoch(self._data, n_rows, order, order.numel(), batch_size)
