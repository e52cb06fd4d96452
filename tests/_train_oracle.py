"""float64 restatement of `train`'s step — the yardstick of po_train.hip.  The Keras layers are restated in torch (the
semantics tests/_call_oracle.py writes out) and differentiated by torch autograd, so the gradients do not share the
kernels' hand derivation.  The CTC loss is the α recursion in log space:
  merge_repeated = False (tf ctc_loss's ctc_merge_repeated=False, the reference's default): a path's labels are its
    non-blank frames; label states do not self-loop and a blank may always be skipped
  merge_repeated = True: standard CTC (repeats merged, then blanks removed; a blank is needed between equal labels)
Blank is class 4; the softmax is inside the loss.  Adam is Keras' (ResourceApplyAdam's) update, restated in float64."""
import itertools

import numpy as np
import torch

NEG = -1e30     # log 0 with finite gradients


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def gru(x, W, U, b, go_backwards=False):
    """x (n, T, Cin) -> (n, T, H) in processing order (Keras GRU, reset_after=True, gates z, r, h)"""
    H = U.shape[0]
    if go_backwards:
        x = torch.flip(x, [1])
    P = x @ W + b[0]
    h = torch.zeros(x.shape[0], H, dtype=x.dtype)
    out = []
    for t in range(x.shape[1]):
        rec = h @ U + b[1]
        z = torch.sigmoid(P[:, t, :H] + rec[:, :H])
        r = torch.sigmoid(P[:, t, H:2 * H] + rec[:, H:2 * H])
        hh = torch.tanh(P[:, t, 2 * H:] + r * rec[:, 2 * H:])
        h = z * h + (1 - z) * hh
        out.append(h)
    return torch.stack(out, 1)


def conv1d_relu(x, W, b):
    K, T = W.shape[0], x.shape[1]
    pl = (K - 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, pl, K - 1 - pl))
    return torch.relu(sum(xp[:, j:j + T] @ W[j] for j in range(K)) + b)


def forward(layers, params, windows):
    """logits (n, T, 5) of windows (n, T); layers: [(kind, number of tensors)], params: the tensors in order"""
    x = _t(windows)[:, :, None]
    k = 0
    for kind, nt in layers:
        p = params[k:k + nt]
        k += nt
        if kind == "conv":
            x = conv1d_relu(x, *p)
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


def ctc_nll(logp, label, merge_repeated=False):
    """-log P(label | frames) of log-probabilities logp (T, 5) (a torch tensor, differentiable)"""
    T = logp.shape[0]
    L = len(label)
    S = 2 * L + 1
    lab = [4 if s % 2 == 0 else int(label[s // 2]) for s in range(S)]
    idx = torch.tensor(lab)
    self_ok = torch.tensor([s % 2 == 0 or merge_repeated for s in range(S)])
    skip_ok = torch.tensor([s % 2 == 1 and s >= 3 and (not merge_repeated or lab[s] != lab[s - 2]) for s in range(S)])
    neg = torch.full((S,), NEG, dtype=logp.dtype)
    a = neg.clone()
    a = torch.where(torch.arange(S) == 0, logp[0, 4], a)
    if S > 1:
        a = torch.where(torch.arange(S) == 1, logp[0, lab[1]], a)
    for t in range(1, T):
        stay = torch.where(self_ok, a, neg)
        one = torch.cat([neg[:1], a[:-1]])
        two = torch.where(skip_ok, torch.cat([neg[:2], a[:-2]]) if S > 2 else neg, neg)
        a = torch.logsumexp(torch.stack([stay, one, two]), 0) + logp[t, idx]
    return -(torch.logsumexp(a[-2:], 0) if S > 1 else a[0])


def _flat_params(net):
    return [_t(t).requires_grad_(True) for l in net.layers for t in l.tensors]


def loss_and_grad(net, windows, labels, merge_repeated=False):
    """(per-window losses (n,), gradient of their mean in po_call_batch's flat layout, logits (n, T, 5), dloss/dlogits)"""
    params = _flat_params(net)
    layers = [(l.kind, len(l.tensors)) for l in net.layers]
    logits = forward(layers, params, windows)
    logits.retain_grad()
    lp = torch.log_softmax(logits, 2)
    losses = torch.stack([ctc_nll(lp[i], labels[i], merge_repeated) for i in range(len(labels))])
    losses.mean().backward()
    g = np.concatenate([p.grad.numpy().ravel() for p in params])
    return losses.detach().numpy(), g, logits.detach().numpy(), logits.grad.numpy()


def ctc_from_logits(logits, labels, merge_repeated=False):
    """(losses (n,), dmean/dlogits (n, T, 5)) of given logits (n, T, 5)"""
    lg = _t(logits).requires_grad_(True)
    lp = torch.log_softmax(lg, 2)
    losses = torch.stack([ctc_nll(lp[i], labels[i], merge_repeated) for i in range(len(labels))])
    losses.mean().backward()
    return losses.detach().numpy(), lg.grad.numpy()


def brute_nll(logp, label, merge_repeated=False):
    """-log of the summed probability of every path of T frames whose labelling is `label` (T <= 6)"""
    logp = np.asarray(logp, dtype=np.float64)
    T = logp.shape[0]
    want = tuple(int(c) for c in label)
    tot = 0.0
    for path in itertools.product(range(5), repeat=T):
        seq = path
        if merge_repeated:
            seq = [c for i, c in enumerate(path) if i == 0 or c != path[i - 1]]
        if tuple(c for c in seq if c != 4) == want:
            tot += np.exp(sum(logp[t, c] for t, c in enumerate(path)))
    return -np.log(tot)


def adam(p, grads, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
    """p after Keras Adam steps with the given gradients, float64"""
    p = np.asarray(p, dtype=np.float64).copy()
    m = np.zeros_like(p)
    v = np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, dtype=np.float64)
        m += (g - m) * (1 - beta1)
        v += (g * g - v) * (1 - beta2)
        p -= lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m / (np.sqrt(v) + eps)
    return p
