"""float64 restatement of the Keras models of the reference's build_model (network.py:15-55) — the yardstick of `call`
(no recorded reference output of the network exists).  Keras semantics, written out:
  Conv1D(padding='same', stride 1): out[t] = relu(bias + sum_j x[t + j - (K-1)//2] @ W[j]), zeros outside the window
  GRU(reset_after=True): gates z, r, h; h~ = tanh(x W_h + b_in,h + r * (h U_h + b_rec,h)); h' = z h + (1 - z) h~
  Bidirectional(concat): [forward, backward], the backward outputs put back into forward time order
  GRU(go_backwards=True, return_sequences=True): walks the reversed input and returns its outputs in that reversed order
  Dense(5), then softmax."""
import numpy as np


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def gru(x, W, U, b, go_backwards=False):
    """x (n, T, Cin) -> (n, T, H) in processing order"""
    W, U, b = (np.asarray(a, dtype=np.float64) for a in (W, U, b))
    H = U.shape[0]
    if go_backwards:
        x = x[:, ::-1]
    P = x @ W + b[0]
    h = np.zeros((x.shape[0], H))
    out = np.empty((x.shape[0], x.shape[1], H))
    for t in range(x.shape[1]):
        rec = h @ U + b[1]
        z = _sigmoid(P[:, t, :H] + rec[:, :H])
        r = _sigmoid(P[:, t, H:2 * H] + rec[:, H:2 * H])
        hh = np.tanh(P[:, t, 2 * H:] + r * rec[:, 2 * H:])
        h = z * h + (1 - z) * hh
        out[:, t] = h
    return out


def conv1d_relu(x, W, b):
    W = np.asarray(W, dtype=np.float64)
    K = W.shape[0]
    pl = (K - 1) // 2
    T = x.shape[1]
    xp = np.zeros((x.shape[0], T + K - 1, x.shape[2]))
    xp[:, pl:pl + T] = x
    out = sum(xp[:, j:j + T] @ W[j] for j in range(K)) + np.asarray(b, dtype=np.float64)
    return np.maximum(out, 0.0)


def forward(net, windows):
    """(logits, probs), each (n, T, 5) float64, of `windows` (n, T) through a poreover_amd.network.checkpoint.Network"""
    x = np.asarray(windows, dtype=np.float64)[:, :, None]
    for l in net.layers:
        if l.kind == "conv":
            x = conv1d_relu(x, *l.tensors)
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
    """(logits, probs) of one scaled signal, (len(signal), 5), windows as the reference cuts them"""
    n = max(1, -(-len(signal) // window))
    pad = np.zeros(n * window)
    pad[:len(signal)] = signal
    lg, pr = forward(net, pad.reshape(n, window))
    return lg.reshape(-1, 5)[:len(signal)], pr.reshape(-1, 5)[:len(signal)]


def greedy(probs):
    """CTC best-path string of (T, 5) probabilities, blank last"""
    a = np.argmax(probs, axis=1)
    keep = np.concatenate([[True], a[1:] != a[:-1]]) & (a != 4)
    return "".join("ACGT"[i] for i in a[keep])
