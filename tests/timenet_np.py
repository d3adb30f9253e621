"""The time-allocation network restated in numpy (float32 or float64), independent of the HIP kernels and of torch: what the
GPU tests compare against where the reference left no recorded output (seeded random weights, L = 10), and what the CPU test
checks against the recorded outputs of the reference's model (tests/golden/timenet_seq5_cases.npz).

    state  (B, 9, 2)     -> Conv1d(9->8, k 3, pad 1) -> ReLU -> MaxPool1d(2) -> Linear(8->6)
    hpolys (B, 50, 4, L) -> Conv2d(50->16, 3x3, pad 1) -> ReLU -> MaxPool2d(2) -> MaxPool2d(2) -> Flatten -> Linear(->32)
    x = [6 | 32], the same at every step;  h = c = 0;  L steps of an LSTM cell (hidden 256, gates i, f, g, o);
    tf_k = w_t . h + b_t,  stop_k = sigmoid(w_s . h + b_s);  count = 1 + first k with stop_k > threshold (L if none).
"""
import os

import numpy as np

# the tensors of the model in the order the weights file and anet_timenet_create take them, with the state-dict names
KEYS = ["state_input_module.0.weight", "state_input_module.0.bias", "state_input_module.4.weight", "state_input_module.4.bias",
        "hpoly_input_module.0.weight", "hpoly_input_module.0.bias", "hpoly_input_module.5.weight", "hpoly_input_module.5.bias",
        "output_module.weight_ih_l0", "output_module.weight_hh_l0", "output_module.bias_ih_l0", "output_module.bias_hh_l0",
        "tfs_output_layer.weight", "tfs_output_layer.bias", "stop_token_output_layer.0.weight", "stop_token_output_layer.0.bias"]


def shapes(seq_len, hidden=256):
    flat = 16 * (seq_len // 4)
    return [(8, 9, 3), (8,), (6, 8), (6,), (16, 50, 3, 3), (16,), (32, flat), (32,), (4 * hidden, 38), (4 * hidden, hidden),
            (4 * hidden,), (4 * hidden,), (1, hidden), (1,), (1, hidden), (1,)]


def random_weights(seq_len, seed, hidden=256):
    """Seeded weights at the scale torch's default initialisation gives (uniform in +-1/sqrt(fan_in))."""
    rng = np.random.default_rng(seed)
    fan = [27, 27, 8, 8, 450, 450, 16 * (seq_len // 4), 16 * (seq_len // 4), hidden, hidden, hidden, hidden, hidden, hidden,
           hidden, hidden]
    return {k: (rng.uniform(-1.0, 1.0, s) / np.sqrt(f)).astype(np.float32) for k, s, f in zip(KEYS, shapes(seq_len, hidden), fan)}


def load_golden_weights(directory):
    """The weights recorded under tests/golden/timenet_seq5/: one .npy per tensor, weight_hh_l0 split by gate."""
    out = {}
    for k in KEYS:
        if k == "output_module.weight_hh_l0":
            out[k] = np.concatenate([np.load(os.path.join(directory, f"{k}.gate{g}.npy"), allow_pickle=False) for g in range(4)])
        else:
            out[k] = np.load(os.path.join(directory, k + ".npy"), allow_pickle=False)
    return out


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def encode(w, state, hpolys, dtype=np.float64):
    """The 38-vector x of every problem: (B, 38)."""
    W = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    state = np.asarray(state, dtype=dtype); hp = np.asarray(hpolys, dtype=dtype)
    B, L = state.shape[0], hp.shape[3]
    # Conv1d over the length-2 signal, pad 1: out[o, t] = b[o] + sum_{c, k} w[o, c, k] in[c, t + k - 1]
    sp = np.zeros((B, 9, 4), dtype=dtype); sp[:, :, 1:3] = state
    cw = W[KEYS[0]]
    conv = np.stack([np.einsum("ock,bck->bo", cw, sp[:, :, t:t + 3]) for t in range(2)], axis=-1) + W[KEYS[1]][None, :, None]
    pooled = np.maximum(conv, 0).max(axis=-1)                                  # ReLU, MaxPool1d(2): (B, 8)
    se = pooled @ W[KEYS[2]].T + W[KEYS[3]]
    # Conv2d over (4, L), pad 1
    pp = np.zeros((B, 50, 6, L + 2), dtype=dtype); pp[:, :, 1:5, 1:L + 1] = hp
    kw = W[KEYS[4]]
    c2 = np.zeros((B, 16, 4, L), dtype=dtype)
    for dy in range(3):
        for dx in range(3):
            c2 += np.einsum("oc,bchw->bohw", kw[:, :, dy, dx], pp[:, :, dy:dy + 4, dx:dx + L])
    c2 = np.maximum(c2 + W[KEYS[5]][None, :, None, None], 0)
    w1 = L // 2
    p1 = c2[:, :, :, :2 * w1].reshape(B, 16, 2, 2, w1, 2).max(axis=(3, 5))      # (B, 16, 2, L // 2)
    w2 = w1 // 2
    p2 = p1[:, :, :, :2 * w2].reshape(B, 16, 1, 2, w2, 2).max(axis=(3, 5))      # (B, 16, 1, L // 4)
    he = p2.reshape(B, 16 * w2) @ W[KEYS[6]].T + W[KEYS[7]]
    return np.concatenate([se, he], axis=1).astype(dtype)


def forward(w, state, hpolys, threshold=0.5, dtype=np.float64):
    """times (B, L), count (B,) int32, tf (B, L), stop (B, L) in `dtype`."""
    x = encode(w, state, hpolys, dtype)
    W = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    B, L = x.shape[0], np.asarray(hpolys).shape[3]
    H = W[KEYS[9]].shape[1]
    gx = x @ W[KEYS[8]].T + W[KEYS[10]] + W[KEYS[11]]
    h = np.zeros((B, H), dtype=dtype); c = np.zeros((B, H), dtype=dtype)
    tf = np.zeros((B, L), dtype=dtype); stop = np.zeros((B, L), dtype=dtype)
    for k in range(L):
        g = gx + h @ W[KEYS[9]].T
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = (f * c + i * gg).astype(dtype)
        h = (o * np.tanh(c)).astype(dtype)
        tf[:, k] = h @ W[KEYS[12]][0] + W[KEYS[13]][0]
        stop[:, k] = _sigmoid(h @ W[KEYS[14]][0] + W[KEYS[15]][0])
    count, times = count_times(tf, stop, threshold)
    return times, count, tf, stop


def count_times(tf, stop, threshold):
    """count = 1 + first k with stop_k > threshold (L if none); times = tf[:count], zero after."""
    tf = np.asarray(tf); stop = np.asarray(stop)
    L = tf.shape[1]
    over = stop.astype(np.float64) > float(threshold)          # the export compares the float32 token, widened, with a double
    count = np.where(over.any(axis=1), over.argmax(axis=1) + 1, L).astype(np.int32)
    times = np.where(np.arange(L)[None, :] < count[:, None], tf, 0).astype(tf.dtype)
    return count, times


def stop_margin(stop, threshold):
    """min_k |stop_k - threshold| per case: a case may be left out of the count / times comparison only below 1e-4."""
    return np.abs(np.asarray(stop, dtype=np.float64) - threshold).min(axis=1)
