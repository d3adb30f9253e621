"""The time-allocation network of the planner (minsnap_network_conv_lstm.py:37-88, 114-187) on the device: weights handle and
batched inference.  All arithmetic runs in the HIP kernels of csrc/timenet_kernels.h behind anet_timenet_*; nothing here
computes the network on the host.

    net = TimeAllocNet.load("seq5.anetw")            # or from_state_dict / from_torchscript
    times, count = net.forward(state, hpolys)         # state (B, 9, 2), hpolys (B, 50, 4, L): `pack_model_inputs`, stacked

Weights file (little-endian): 8 bytes b"ANETTIME", uint32 version (1), uint32 seq_len, uint32 hidden, then the 16 tensors of the
state dict as float32 in the order of TENSOR_KEYS with their natural shapes.  include/allocnet_amd/time_net.hpp reads the same file.
"""
import ctypes
import struct

import numpy as np

from .context import default_context

MAGIC = b"ANETTIME"
VERSION = 1
TENSOR_KEYS = ("state_input_module.0.weight", "state_input_module.0.bias", "state_input_module.4.weight",
               "state_input_module.4.bias", "hpoly_input_module.0.weight", "hpoly_input_module.0.bias",
               "hpoly_input_module.5.weight", "hpoly_input_module.5.bias", "output_module.weight_ih_l0",
               "output_module.weight_hh_l0", "output_module.bias_ih_l0", "output_module.bias_hh_l0", "tfs_output_layer.weight",
               "tfs_output_layer.bias", "stop_token_output_layer.0.weight", "stop_token_output_layer.0.bias")
KEEP_PADDING, FORM_SINGLE, FORM_TILE = 1, 2, 4        # ANET_TIMENET_* flags
SINGLE_MAX = 1024                                     # ANET_TIMENET_SINGLE_MAX: batches up to this take the single form


def tensor_shapes(seq_len, hidden=256):
    flat = 16 * (seq_len // 4)
    return ((8, 9, 3), (8,), (6, 8), (6,), (16, 50, 3, 3), (16,), (32, flat), (32,), (4 * hidden, 38), (4 * hidden, hidden),
            (4 * hidden,), (4 * hidden,), (1, hidden), (1,), (1, hidden), (1,))


class TimeAllocNet:
    """The exported model's layers with its weights; `forward` is the whole model for a batch."""

    def __init__(self, weights, ctx=None):
        w = {k: np.ascontiguousarray(np.asarray(weights[k]), dtype="<f4") for k in TENSOR_KEYS}
        flat = w[TENSOR_KEYS[6]].shape[-1] if w[TENSOR_KEYS[6]].ndim == 2 else -1
        hidden = w[TENSOR_KEYS[9]].shape[-1] if w[TENSOR_KEYS[9]].ndim == 2 else -1
        seq_len = {16: 5, 32: 10}.get(flat)
        if seq_len is None:
            raise ValueError("hpoly_input_module.5.weight must be (32, 16) [seq_len 5] or (32, 32) [seq_len 10]")
        for k, s in zip(TENSOR_KEYS, tensor_shapes(seq_len, hidden)):
            if w[k].shape != s:
                raise ValueError(f"{k}: shape {w[k].shape}, expected {s}")
        self.weights, self.seq_len, self.hidden = w, seq_len, hidden
        self._ctx, self._handle = ctx, None

    # ---- construction -----------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, ctx=None):
        """sd: the 16 tensors by their state-dict names (numpy arrays or CPU torch tensors)."""
        conv = lambda v: v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        missing = [k for k in TENSOR_KEYS if k not in sd]
        if missing:
            raise ValueError(f"state dict lacks {missing}")
        return cls({k: conv(sd[k]) for k in TENSOR_KEYS}, ctx)

    @classmethod
    def from_torchscript(cls, path, ctx=None):
        """The weights of an exported model (the planner's .pt).  The module is only read, never run."""
        import torch
        return cls.from_state_dict(torch.jit.load(path, map_location="cpu").state_dict(), ctx)

    @classmethod
    def load(cls, path, ctx=None):
        with open(path, "rb") as f:
            buf = f.read()
        if len(buf) < 20 or buf[:8] != MAGIC:
            raise ValueError(f"{path}: not a time-allocation weights file")
        version, seq_len, hidden = struct.unpack("<III", buf[8:20])
        if version != VERSION or seq_len not in (5, 10) or hidden < 1 or hidden > 4096:
            raise ValueError(f"{path}: version {version}, seq_len {seq_len}, hidden {hidden} not supported")
        shapes = tensor_shapes(seq_len, hidden)
        if len(buf) != 20 + 4 * sum(int(np.prod(s)) for s in shapes):
            raise ValueError(f"{path}: {len(buf)} bytes, the header announces another size")
        w, off = {}, 20
        for k, s in zip(TENSOR_KEYS, shapes):
            n = int(np.prod(s))
            w[k] = np.frombuffer(buf, dtype="<f4", count=n, offset=off).reshape(s).copy()
            off += 4 * n
        return cls(w, ctx)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(MAGIC + struct.pack("<III", VERSION, self.seq_len, self.hidden))
            for k in TENSOR_KEYS:
                f.write(self.weights[k].astype("<f4", copy=False).tobytes())

    # ---- device handle ----------------------------------------------------------------------------
    def _net(self, ctx=None):
        if self._handle is None:
            self._ctx = ctx or self._ctx or default_context()
            arrs = [self.weights[k].astype(np.float32, copy=False) for k in TENSOR_KEYS]
            ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            h = ctypes.c_void_p()
            self._ctx.check(self._ctx.lib.anet_timenet_create(self._ctx.handle, self.seq_len, self.hidden, ptrs, ctypes.byref(h)))
            self._handle = h
        return self._handle

    @property
    def device_bytes(self):
        """anet_timenet_device_bytes: device memory the handle holds (weights, workspace, staging)."""
        return int(self._ctx.lib.anet_timenet_device_bytes(self._handle)) if self._handle is not None else 0

    def close(self):
        if self._handle is not None:
            self._ctx.lib.anet_timenet_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inference --------------------------------------------------------------------------------
    @staticmethod
    def _flags(skip_padding, form):
        if form not in (None, "single", "tile"):
            raise ValueError("form: None, 'single' or 'tile'")
        return (0 if skip_padding else KEEP_PADDING) | {None: 0, "single": FORM_SINGLE, "tile": FORM_TILE}[form]

    def forward(self, state, hpolys, threshold=0.5, steps=False, skip_padding=True, form=None):
        """state (B, 9, 2), hpolys (B, 50, 4, L) -- one problem may come without the batch axis.  numpy in: numpy out through
        anet_timenet_forward; torch device tensors in: `forward_dev`.  Returns times (B, L) float32 (zero after count) and count
        (B,) int32; with steps=True also tf, stop (B, L) of all L steps.
        form: None = by batch size (up to SINGLE_MAX problems a workgroup each, above it tiles of 32 on the matrix instruction);
        skip_padding=False computes the products with the zero padding too (the same bits; kept for the test)."""
        if hasattr(state, "is_cuda"):
            return self.forward_dev(state, hpolys, threshold, steps, skip_padding, form)
        L = self.seq_len
        st = np.ascontiguousarray(state, dtype=np.float32); hp = np.ascontiguousarray(hpolys, dtype=np.float32)
        one = st.ndim == 2
        if one:
            st, hp = st[None], hp[None]
        B = st.shape[0]
        if st.shape != (B, 9, 2) or hp.shape != (B, 50, 4, L):
            raise ValueError(f"state (B, 9, 2) and hpolys (B, 50, 4, {L}) expected, got {st.shape} and {hp.shape}")
        net = self._net()
        times = np.zeros((B, L), dtype=np.float32); count = np.zeros(B, dtype=np.int32)
        tf = np.zeros((B, L), dtype=np.float32) if steps else None
        stop = np.zeros((B, L), dtype=np.float32) if steps else None
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        self._ctx.check(self._ctx.lib.anet_timenet_forward(self._ctx.handle, net, L, B, p(st), p(hp), float(threshold),
                                                           self._flags(skip_padding, form), p(times), p(tf), p(stop), p(count)))
        out = (times, count, tf, stop) if steps else (times, count)
        return tuple(a[0] for a in out) if one else out

    def forward_dev(self, state, hpolys, threshold=0.5, steps=False, skip_padding=True, form=None, stream=None, out=None):
        """anet_timenet_forward_dev: float32 contiguous torch device tensors state (B, 9, 2), hpolys (B, 50, 4, L); asynchronous
        on `stream` (default: torch's current stream); returns device tensors as `forward`.  out: an earlier result of the same
        shapes to write into (then the call allocates nothing after the first one at a batch size)."""
        import torch
        L = self.seq_len
        B = state.shape[0]
        for t, s in ((state, (B, 9, 2)), (hpolys, (B, 50, 4, L))):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == s):
                raise ValueError(f"float32 contiguous device tensors state (B, 9, 2), hpolys (B, 50, 4, {L}) expected")
        net = self._net(default_context(state.device.index or 0) if self._ctx is None else None)
        if out is None:
            new = lambda dt: torch.empty((B, L), device=state.device, dtype=dt)
            out = (new(torch.float32), torch.empty(B, device=state.device, dtype=torch.int32)) + \
                ((new(torch.float32), new(torch.float32)) if steps else ())
        times, count = out[0], out[1]
        tf, stop = (out[2], out[3]) if steps else (None, None)
        st = stream if stream is not None else torch.cuda.current_stream(state.device).cuda_stream
        q = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        self._ctx.check(self._ctx.lib.anet_timenet_forward_dev(self._ctx.handle, net, L, B, q(state), q(hpolys), float(threshold),
                                                               self._flags(skip_padding, form), q(times), q(tf), q(stop), q(count),
                                                               ctypes.c_void_p(st)))
        return out
