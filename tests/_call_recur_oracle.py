"""The float64 yardstick of `--recurrence bf16x3`: _call_oracle's forward with the recurrence's product h @ U taken as
hh @ Uh + hl @ Uh + hh @ Ul, the operands split by network.split_bf16 (h is taken to float32 first, as the device holds it);
the products and sums, the bias, the gates, the input projection, Conv1D, Dense and the softmax stay float64.  With
proj="bf16" the input projection is _call_bf16_oracle's (`--precision bf16` together with `--recurrence bf16x3`).  It wraps
_call_oracle and leaves it as it is."""
import numpy as np

import _call_bf16_oracle as OB
import _call_oracle as O
from poreover_amd.network import split_bf16


def split_product(h, Uh, Ul):
    """hh @ Uh + hl @ Uh + hh @ Ul in float64; Uh, Ul float64 arrays of a split U"""
    hh, hl = (a.astype(np.float64) for a in split_bf16(np.asarray(h, dtype=np.float32)))
    return hh @ Uh + hl @ Uh + hh @ Ul


def gru(x, W, U, b, go_backwards=False, proj="f32"):
    """_call_oracle.gru with the recurrent product on split bf16 operands"""
    b = np.asarray(b, dtype=np.float64)
    Uh, Ul = (a.astype(np.float64) for a in split_bf16(U))
    H = Uh.shape[0]
    if go_backwards:
        x = x[:, ::-1]
    P = OB.proj(x, W, b[0]) if proj == "bf16" else x @ np.asarray(W, dtype=np.float64) + b[0]
    h = np.zeros((x.shape[0], H))
    out = np.empty((x.shape[0], x.shape[1], H))
    for t in range(x.shape[1]):
        rec = split_product(h, Uh, Ul) + b[1]
        z = O._sigmoid(P[:, t, :H] + rec[:, :H])
        r = O._sigmoid(P[:, t, H:2 * H] + rec[:, H:2 * H])
        hh = np.tanh(P[:, t, 2 * H:] + r * rec[:, 2 * H:])
        h = z * h + (1 - z) * hh
        out[:, t] = h
    return out


def forward(net, windows, proj="f32"):
    """(logits, probs), each (n, T, 5) float64: _call_oracle.forward with the GRU layers above"""
    x = np.asarray(windows, dtype=np.float64)[:, :, None]
    for l in net.layers:
        if l.kind == "conv":
            x = O.conv1d_relu(x, *l.tensors)
        elif l.kind == "bigru":
            f = gru(x, *l.tensors[:3], proj=proj)
            bk = gru(x, *l.tensors[3:], go_backwards=True, proj=proj)[:, ::-1]
            x = np.concatenate([f, bk], axis=2)
        elif l.kind == "gru":
            x = gru(x, *l.tensors, proj=proj)
        elif l.kind == "gru_back":
            x = gru(x, *l.tensors, go_backwards=True, proj=proj)
        elif l.kind == "dense":
            x = x @ np.asarray(l.tensors[0], dtype=np.float64) + np.asarray(l.tensors[1], dtype=np.float64)
    e = np.exp(x - x.max(axis=2, keepdims=True))
    return x, e / e.sum(axis=2, keepdims=True)


def basecall(net, signal, window, proj="f32"):
    """_call_oracle.basecall through the forward above"""
    n = max(1, -(-len(signal) // window))
    pad = np.zeros(n * window)
    pad[:len(signal)] = signal
    lg, pr = forward(net, pad.reshape(n, window), proj=proj)
    return lg.reshape(-1, 5)[:len(signal)], pr.reshape(-1, 5)[:len(signal)]
