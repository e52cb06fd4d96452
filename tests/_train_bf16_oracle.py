"""The float64 yardstick of a bf16-mode trainer (po_train_set_precision(PO_CALL_BF16)): _train_oracle's step
with two torch.autograd.Functions in the GRU.
  projection         forward round(x) @ round(W); backward dW = round(x)ᵀ @ round(dP), dx = round(dP) @ round(W)ᵀ
  recurrent product  forward h @ U exact; backward dh = d @ Uᵀ exact, dU = round(h)ᵀ @ round(d)
round is round_bf16 after a cast to float32, as the device holds the values.  Everything else is _train_oracle's and is
imported from it unchanged: the bias gradients (exact sums of the unrounded dP and d), Conv1D, Dense, the CTC loss, the flat
layout."""
import numpy as np
import torch

import _train_oracle as O
from poreover_amd.network import round_bf16


def _r(t):
    """a float64 tensor rounded to bf16 through float32"""
    return torch.from_numpy(round_bf16(t.detach().numpy().astype(np.float32)).astype(np.float64))


class Proj(torch.autograd.Function):
    """x (n, T, cin) @ W (cin, G) on bf16 operands, forward and backward"""

    @staticmethod
    def forward(ctx, x, W):
        xr, Wr = _r(x), _r(W)
        ctx.save_for_backward(xr, Wr)
        return xr @ Wr

    @staticmethod
    def backward(ctx, dP):
        xr, Wr = ctx.saved_tensors
        dr = _r(dP)
        dW = xr.reshape(-1, xr.shape[-1]).T @ dr.reshape(-1, dr.shape[-1])
        return dr @ Wr.T, dW


class Rec(torch.autograd.Function):
    """h (n, H) @ U (H, G): exact forward and dh, dU on bf16 operands"""

    @staticmethod
    def forward(ctx, h, U):
        ctx.save_for_backward(h, U)
        return h @ U

    @staticmethod
    def backward(ctx, d):
        h, U = ctx.saved_tensors
        return d @ U.T, _r(h).T @ _r(d)


def gru(x, W, U, b, go_backwards=False):
    """_train_oracle.gru with the two products above"""
    H = U.shape[0]
    if go_backwards:
        x = torch.flip(x, [1])
    P = Proj.apply(x, W) + b[0]
    h = torch.zeros(x.shape[0], H, dtype=x.dtype)
    out = []
    for t in range(x.shape[1]):
        rec = Rec.apply(h, U) + b[1]
        z = torch.sigmoid(P[:, t, :H] + rec[:, :H])
        r = torch.sigmoid(P[:, t, H:2 * H] + rec[:, H:2 * H])
        hh = torch.tanh(P[:, t, 2 * H:] + r * rec[:, 2 * H:])
        h = z * h + (1 - z) * hh
        out.append(h)
    return torch.stack(out, 1)


def forward(layers, params, windows):
    """_train_oracle.forward with the GRU layers above"""
    x = O._t(windows)[:, :, None]
    k = 0
    for kind, nt in layers:
        p = params[k:k + nt]
        k += nt
        if kind == "conv":
            x = O.conv1d_relu(x, *p)
        elif kind == "bigru":
            f = gru(x, *p[:3])
            bk = torch.flip(gru(x, *p[3:], go_backwards=True), [1])
            x = torch.cat([f, bk], 2)
        elif kind == "gru":
            x = gru(x, *p)
        elif kind == "gru_back":
            x = gru(x, *p, go_backwards=True)
        elif kind == "dense":
            x = x @ p[0] + p[1]
    return x


def loss_and_grad(net, windows, labels, merge_repeated=False):
    """_train_oracle.loss_and_grad's four results for the bf16-mode step"""
    params = O._flat_params(net)
    layers = [(l.kind, len(l.tensors)) for l in net.layers]
    logits = forward(layers, params, windows)
    logits.retain_grad()
    lp = torch.log_softmax(logits, 2)
    losses = torch.stack([O.ctc_nll(lp[i], labels[i], merge_repeated) for i in range(len(labels))])
    losses.mean().backward()
    g = np.concatenate([p.grad.numpy().ravel() for p in params])
    return losses.detach().numpy(), g, logits.detach().numpy(), logits.grad.numpy()
