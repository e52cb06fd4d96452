"""The float64 yardstick of `--precision bf16`: _call_oracle's forward with round_bf16 applied to x and W of every GRU
input projection x @ W (the products and sums, the bias, the recurrence, Conv1D, Dense and the softmax stay float64).  It
wraps _call_oracle and leaves it as it is."""
import numpy as np

import _call_oracle as O
from poreover_amd.network import round_bf16


def proj(x, W, b_in):
    """round_bf16(x) @ round_bf16(W) + b_in in float64 (x is taken to float32 first, as the device holds it)"""
    return round_bf16(np.asarray(x, dtype=np.float32)).astype(np.float64) @ round_bf16(W).astype(np.float64) + \
        np.asarray(b_in, dtype=np.float64)


def gru(x, W, U, b, go_backwards=False):
    """_call_oracle.gru with the input projection on bf16 operands"""
    U, b = (np.asarray(a, dtype=np.float64) for a in (U, b))
    H = U.shape[0]
    if go_backwards:
        x = x[:, ::-1]
    P = proj(x, W, b[0])
    h = np.zeros((x.shape[0], H))
    out = np.empty((x.shape[0], x.shape[1], H))
    for t in range(x.shape[1]):
        rec = h @ U + b[1]
        z = O._sigmoid(P[:, t, :H] + rec[:, :H])
        r = O._sigmoid(P[:, t, H:2 * H] + rec[:, H:2 * H])
        hh = np.tanh(P[:, t, 2 * H:] + r * rec[:, 2 * H:])
        h = z * h + (1 - z) * hh
        out[:, t] = h
    return out


def forward(net, windows):
    """(logits, probs), each (n, T, 5) float64: _call_oracle.forward with the GRU layers above"""
    x = np.asarray(windows, dtype=np.float64)[:, :, None]
    for l in net.layers:
        if l.kind == "conv":
            x = O.conv1d_relu(x, *l.tensors)
        elif l.kind == "bigru":
            f = gru(x, *l.tensors[:3])
            bk = gru(x, *l.tensors[3:], go_backwards=True)[:, ::-1]
            x = np.concatenate([f, bk], axis=2)
        elif l.kind == "gru":
            x = gru(x, *l.tensors)
        elif l.kind == "gru_back":
            x = gru(x, *l.tensors, go_backwards=True)
        elif l.kind == "dense":
            x = x @ np.asarray(l.tensors[0], dtype=np.float64) + np.asarray(l.tensors[1], dtype=np.float64)
    e = np.exp(x - x.max(axis=2, keepdims=True))
    return x, e / e.sum(axis=2, keepdims=True)


def basecall(net, signal, window):
    """_call_oracle.basecall through the forward above"""
    n = max(1, -(-len(signal) // window))
    pad = np.zeros(n * window)
    pad[:len(signal)] = signal
    lg, pr = forward(net, pad.reshape(n, window))
    return lg.reshape(-1, 5)[:len(signal)], pr.reshape(-1, 5)[:len(signal)]
