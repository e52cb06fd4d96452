"""`train`: CTC training of the basecalling network (the reference's network.py:66-179), on the GPU.

The step (forward pass, tf.compat.v1.nn.ctc_loss averaged over the batch, its gradient, Keras Adam) runs in HIP
(poreover_amd/csrc/po_train.hip through a po_trainer handle), and so does the held-out validation (po_train_eval: the
argmax path and its edit distance to the labels); this module does what the reference's host loop does:
loads the .npz, draws the holdout and the batches, runs the schedule, prints the same stderr lines, writes train.log,
model.json and the checkpoints.  Where the reference differs from its own flags, this honours them:
--learning_rate and --ctc_merge_repeated take effect, T is the data's window length, the holdout is fixed for the run,
checkpoints are .npz files of the checkpoint's tensor names next to a TF-style `checkpoint` file.  Beyond the reference,
and off by default: gradient accumulation over several batches, clipping by the global norm with a guard
against non-finite gradients, decoupled weight decay, a learning-rate schedule and Adam's state saved and resumed."""
import ctypes as C
import datetime
import json
import math
import os
import sys

import numpy as np

from .. import _lib
from . import checkpoint as ckpt

__all__ = ["TrainError", "Trainer", "TrainerGroup", "plan_steps", "validation_error_group", "load_data", "check_labels", "plan_batches", "init_weights", "validation_error",
           "validation_error_device", "lr_at", "optimizer_path", "load_optimizer", "train"]

ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-7)     # Keras Adam()'s defaults


class TrainError(ValueError):
    pass


def load_data(path):
    """(signal (N, T) float32, labels int32, row_lengths int32) of a training .npz (to_npz.py's layout), checked"""
    try:
        z = np.load(path)
    except (OSError, ValueError) as e:
        raise TrainError("train: cannot read --data %s: %s" % (path, e))
    with z:
        missing = [k for k in ("signal", "labels", "row_lengths") if k not in z.files]
        if missing:
            raise TrainError("train: %s has no %s array (a training .npz holds signal, labels and row_lengths)" %
                             (path, ", ".join(missing)))
        sig, lab, rl = z["signal"], z["labels"], z["row_lengths"]
    if sig.ndim != 2 or sig.shape[0] < 1 or sig.shape[1] < 1:
        raise TrainError("train: signal has shape %s, not (windows, samples)" % (sig.shape,))
    if rl.ndim != 1 or len(rl) != sig.shape[0]:
        raise TrainError("train: row_lengths has %d entries for %d signal windows" % (rl.size, sig.shape[0]))
    if np.any(rl < 0):
        raise TrainError("train: row_lengths holds a negative length (window %d)" % int(np.argmax(rl < 0)))
    if int(rl.sum()) != lab.size:
        raise TrainError("train: row_lengths sums to %d, labels holds %d values" % (int(rl.sum()), lab.size))
    lab = np.asarray(lab).ravel()
    if lab.size and (not np.all(np.isfinite(lab)) or np.any(lab != np.round(lab))):
        raise TrainError("train: labels must be integers 0..3 (A C G T)")
    lab = lab.astype(np.int64)
    if not np.all(np.isfinite(sig)):
        raise TrainError("train: signal holds NaN or infinite samples")
    return np.ascontiguousarray(sig, dtype=np.float32), lab.astype(np.int32), np.asarray(rl, dtype=np.int32)


def check_labels(labels, row_lengths, T, merge_repeated):
    """refuse labels outside 0..3 and windows whose label cannot fit in T frames, naming the window"""
    bad = np.flatnonzero((labels < 0) | (labels > 3))
    off = np.concatenate([[0], np.cumsum(row_lengths)])
    if bad.size:
        w = int(np.searchsorted(off, bad[0], side="right") - 1)
        raise TrainError("train: window %d has label %d (labels are 0..3 = A C G T)" % (w, int(labels[bad[0]])))
    for w in range(len(row_lengths)):
        l = labels[off[w]:off[w + 1]]
        need = len(l) + (int(np.sum(l[1:] == l[:-1])) if merge_repeated else 0)
        if need > T:
            raise TrainError("train: window %d has %d labels, which need %d frames; windows have %d samples%s" % (
                w, len(l), need, T, " (--ctc_merge_repeated needs a blank between equal labels)" if merge_repeated else ""))


def plan_batches(n_windows, batch_size, holdout, epochs, seed):
    """(holdout batches, [training batches of every epoch]): one seeded permutation; its first validation_size batches are
    held out for the whole run (validation_size = int(int(N / batch_size) * holdout), as the reference), the rest is
    reshuffled every epoch and cut into whole batches (the remainder is dropped)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_windows)
    nval = int(int(n_windows / batch_size) * holdout)
    held = perm[:nval * batch_size].reshape(nval, batch_size)
    rest = perm[nval * batch_size:]
    nb = len(rest) // batch_size
    batches = []
    for _ in range(epochs):
        order = rest[rng.permutation(len(rest))]
        batches.extend(order[:nb * batch_size].reshape(nb, batch_size))
    return held, batches


def _glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, shape)


def _orthogonal(rng, rows, cols):
    """Keras Orthogonal(gain=1) of a (rows, cols) matrix: QR of a normal matrix, signs fixed by diag(R)"""
    a = rng.standard_normal((max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    return q.T if rows < cols else q


def init_weights(model_config, seed=None):
    """{name: array} of Keras' initial weights for an architecture, drawn with numpy from `seed`: glorot_uniform for
    every kernel (Conv1D fan_in = K·cin, fan_out = K·F), orthogonal for each recurrent kernel (H, 3H) — H the architecture's GRU units —, zero biases"""
    spec = ckpt.parse_model_json(model_config)
    rng = np.random.default_rng(seed)
    v = "/.ATTRIBUTES/VARIABLE_VALUE"
    out, cin = {}, 1
    for i, (kind, s) in enumerate(spec):
        p = "layer_with_weights-%d/" % i
        if kind == "conv":
            K, F = s["kernel"], s["filters"]
            out[p + "kernel" + v] = _glorot(rng, (K, cin, F), K * cin, K * F)
            out[p + "bias" + v] = np.zeros(F)
            cin = F
        elif kind == "dense":
            out[p + "kernel" + v] = _glorot(rng, (cin, ckpt.NUM_LABELS), cin, ckpt.NUM_LABELS)
            out[p + "bias" + v] = np.zeros(ckpt.NUM_LABELS)
        else:
            dirs = ["forward_layer/", "backward_layer/"] if kind == "bigru" else [""]
            H = s["units"]
            for d in dirs:
                q = p + d + "cell/"
                out[q + "kernel" + v] = _glorot(rng, (cin, 3 * H), cin, 3 * H)
                out[q + "recurrent_kernel" + v] = _orthogonal(rng, H, 3 * H)
                out[q + "bias" + v] = np.zeros((2, 3 * H))
            cin = H * len(dirs)
    return {k: a.astype(np.float32) for k, a in out.items()}


def _train_precision_code(name):
    if name not in _lib.TRAIN_PRECISIONS:
        raise ValueError("train precision %r (one of %s)" % (name, ", ".join(_lib.TRAIN_PRECISIONS)))
    return _lib.TRAIN_PRECISIONS[name]


class Trainer:
    """a po_trainer: the model's parameters, gradient and Adam state on the device, for batches of up to max_batch
    windows of T samples.  precision "f32" (default) or "bf16": the operands of the GRU layers' weight and input GEMMs
    (po_train_set_precision); a property of this trainer, which _lib.set_call_precision does not touch"""

    def __init__(self, net, max_batch, T, precision="f32"):
        from .network import _layers_array
        code = _train_precision_code(precision)
        self.h = None
        self.lib = _lib.load()
        self.net, self.T, self.max_batch = net, int(T), int(max_batch)
        self._layers = _layers_array(net)
        self.h = self.lib.po_train_create(self._layers, len(net.layers), self.max_batch, self.T)
        if not self.h:
            detail = self.lib.po_last_error()
            raise _lib.EngineError(_lib.E_ARG, "po_train_create", detail.decode() if detail else "")
        self.n_params = net.n_params()
        self.set_params(net.flat_weights())
        if code != _lib.TRAIN_PRECISIONS["f32"]:
            self.set_precision(precision)

    @property
    def precision(self):
        """the trainer's mode, "f32" or "bf16" (po_train_get_precision)"""
        return {v: k for k, v in _lib.TRAIN_PRECISIONS.items()}[int(self.lib.po_train_get_precision(self.h))]

    def set_precision(self, name):
        """po_train_set_precision: "f32" or "bf16"; parameters and Adam's state are kept; a refusal (a model whose GRU
        layers are not 128 units under "bf16") leaves the mode as it was"""
        code = _train_precision_code(name)
        _lib.check(self.lib.po_train_set_precision(self.h, code), "po_train_set_precision")

    def close(self):
        if self.h:
            self.lib.po_train_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, flat):
        """load the parameters (flat layout) and reset Adam"""
        w = np.ascontiguousarray(flat, dtype=np.float32)
        _lib.check(self.lib.po_train_set_params(self.h, w.ctypes.data, w.size), "po_train_set_params")

    def get_params(self):
        w = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self.lib.po_train_get_params(self.h, w.ctypes.data, w.size), "po_train_get_params")
        return w

    def network(self):
        """the current parameters as a Network"""
        return self.net.with_flat(self.get_params())

    def step(self, windows, labels, merge_repeated=False, lr=1e-3, update=True, grad=False, stage_ms=None, **adam):
        """one step on windows (n, T) with labels (a list of n int sequences): per-window losses (n,) float32, and the
        gradient of the batch-mean loss (flat layout) with grad=True; update=False leaves parameters and Adam alone"""
        a = dict(ADAM, **adam)
        x = np.ascontiguousarray(windows, dtype=np.float32)
        n = x.shape[0]
        lens = np.asarray([len(l) for l in labels], dtype=np.int32)
        lab = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).ravel() for l in labels])
                                   if lens.sum() else np.zeros(1, dtype=np.int32), dtype=np.int32)
        loss = np.empty(n, dtype=np.float32)
        g = np.empty(self.n_params, dtype=np.float32) if grad else None
        ms = (C.c_float * len(_lib.TRAIN_STAGES))() if stage_ms is not None else None
        rc = self.lib.po_train_step(self.h, x.ctypes.data, n, lab.ctypes.data, lens.ctypes.data, 1 if merge_repeated else 0,
                                    float(lr), float(a["beta1"]), float(a["beta2"]), float(a["eps"]), 1 if update else 0,
                                    loss.ctypes.data, g.ctypes.data if grad else None, ms)
        _lib.check(rc, "po_train_step")
        if stage_ms is not None:
            for k, name in enumerate(_lib.TRAIN_STAGES):
                stage_ms[name] = stage_ms.get(name, 0.0) + float(ms[k])
        return (loss, g) if grad else loss

    # ---- the recipe: accumulate micro-batches, then apply once
    def accumulate(self, windows, labels, weight, merge_repeated=False, stage_ms=None):
        """po_train_accumulate: step(update=False)'s gradient of the mean loss of these windows, times `weight`, goes into
        the accumulator (overwrites it where it is empty, else is added by fmaf); with weight = n / N over micro-batches of
        N windows in all, the sum is the gradient of the mean loss over the N.  Returns the per-window losses (n,) float32"""
        x = np.ascontiguousarray(windows, dtype=np.float32)
        n = x.shape[0]
        lens = np.asarray([len(l) for l in labels], dtype=np.int32)
        lab = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).ravel() for l in labels])
                                   if lens.sum() else np.zeros(1, dtype=np.int32), dtype=np.int32)
        loss = np.empty(n, dtype=np.float32)
        ms = (C.c_float * len(_lib.TRAIN_STAGES))() if stage_ms is not None else None
        rc = self.lib.po_train_accumulate(self.h, x.ctypes.data, n, lab.ctypes.data, lens.ctypes.data, 1 if merge_repeated else 0,
                                          float(weight), loss.ctypes.data, ms)
        _lib.check(rc, "po_train_accumulate")
        if stage_ms is not None:
            for k, name in enumerate(_lib.TRAIN_STAGES):
                stage_ms[name] = stage_ms.get(name, 0.0) + float(ms[k])
        return loss

    def apply(self, lr=1e-3, clip_norm=0.0, weight_decay=0.0, **adam):
        """po_train_apply: (grad_norm, applied).  grad_norm: the accumulator's global L2 norm before clipping (float64 sums
        in a fixed order); clip_norm > 0 scales the gradient by clip_norm / grad_norm where that is below 1; then AdamW with
        the decoupled decay lr · weight_decay · p.  applied is False where the norm is NaN or infinite: parameters, Adam's
        m, v and step count are then untouched.  The accumulator is empty afterwards either way."""
        a = dict(ADAM, **adam)
        norm, applied = C.c_double(), C.c_int()
        rc = self.lib.po_train_apply(self.h, float(lr), float(a["beta1"]), float(a["beta2"]), float(a["eps"]),
                                     float(weight_decay), float(clip_norm), C.byref(norm), C.byref(applied))
        _lib.check(rc, "po_train_apply")
        return norm.value, bool(applied.value)

    def accum_reset(self):
        """mark the accumulator empty: the next contribution overwrites it"""
        _lib.check(self.lib.po_train_accum_reset(self.h), "po_train_accum_reset")

    def get_accum(self):
        """the accumulated gradient (flat layout); an EngineError (E_ARG) where nothing is accumulated"""
        g = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self.lib.po_train_get_accum(self.h, g.ctypes.data, g.size), "po_train_get_accum")
        return g

    def set_accum(self, g):
        """load the accumulator (flat layout); counts as one contribution"""
        g = np.ascontiguousarray(g, dtype=np.float32)
        _lib.check(self.lib.po_train_set_accum(self.h, g.ctypes.data, g.size), "po_train_set_accum")

    def get_state(self):
        """(m, v, step): Adam's moments (flat layout) and its step count"""
        m = np.empty(self.n_params, dtype=np.float32)
        v = np.empty(self.n_params, dtype=np.float32)
        step = C.c_int64()
        _lib.check(self.lib.po_train_get_state(self.h, m.ctypes.data, v.ctypes.data, m.size, C.byref(step)), "po_train_get_state")
        return m, v, int(step.value)

    def set_state(self, m, v, step):
        """load Adam's moments and step count (after set_params, which resets them)"""
        m = np.ascontiguousarray(m, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if m.size != v.size:
            raise ValueError("set_state: m has %d values, v %d" % (m.size, v.size))
        _lib.check(self.lib.po_train_set_state(self.h, m.ctypes.data, v.ctypes.data, m.size, int(step)), "po_train_set_state")

    def evaluate(self, windows, labels, merge_repeated=False, loss=True, predictions=False, stage_ms=None):
        """held-out validation of windows (n, T) with labels (a list of n int sequences) on the resident parameters
        (po_train_eval; no gradient, no update): a dict of edit (n,) int32, the edit distance of each window's argmax path
        (classes 0..3 in frame order, repeats kept) to its labels; pred_len (n,) int32, the paths' lengths; status (n,)
        int32, 0 or E_CAP (edit -1) where path and label are both longer than EDIT_MAX_SHORT; with loss=True loss (n,)
        float32, step(update=False)'s bits; with predictions=True pred, a list of n uint8 arrays of codes 0..3"""
        x = np.ascontiguousarray(windows, dtype=np.float32)
        n = x.shape[0]
        lens = np.asarray([len(l) for l in labels], dtype=np.int32)
        lab = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).ravel() for l in labels])
                                   if lens.sum() else np.zeros(1, dtype=np.int32), dtype=np.int32)
        edit, plen, st = (np.empty(n, dtype=np.int32) for _ in range(3))
        ls = np.empty(n, dtype=np.float32) if loss else None
        pred = np.empty((n, self.T), dtype=np.uint8) if predictions else None
        ms = (C.c_float * len(_lib.EVAL_STAGES))() if stage_ms is not None else None
        rc = self.lib.po_train_eval(self.h, x.ctypes.data, n, lab.ctypes.data, lens.ctypes.data, 1 if merge_repeated else 0,
                                    ls.ctypes.data if loss else None, edit.ctypes.data, plen.ctypes.data, st.ctypes.data,
                                    pred.ctypes.data if predictions else None, ms)
        _lib.check(rc, "po_train_eval")
        if stage_ms is not None:
            for k, name in enumerate(_lib.EVAL_STAGES):
                stage_ms[name] = stage_ms.get(name, 0.0) + float(ms[k])
        out = {"edit": edit, "pred_len": plen, "status": st}
        if loss:
            out["loss"] = ls
        if predictions:
            out["pred"] = [pred[w, :plen[w]].copy() for w in range(n)]
        return out

    def last(self, n):
        """(logits, dlogits), each (n, T, 5) float32, of the last step's first n windows"""
        lg = np.empty((n, self.T, ckpt.NUM_LABELS), dtype=np.float32)
        dl = np.empty_like(lg)
        _lib.check(self.lib.po_train_last(self.h, n, lg.ctypes.data, dl.ctypes.data), "po_train_last")
        return lg, dl


def _flat_labels(labels):
    lens = np.asarray([len(l) for l in labels], dtype=np.int32)
    lab = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).ravel() for l in labels])
                               if lens.sum() else np.zeros(1, dtype=np.int32), dtype=np.int32)
    return lens, lab


class TrainerGroup:
    """a po_train_group: len(devices) replicas of a Trainer, replica r on devices[r] (a device may appear
    more than once), each driven by a host thread of its own.  The replicas start from the same parameters and Adam state;
    accumulate() gives each a micro-batch, apply() all-reduces the accumulators in a fixed order (the same bits on every
    replica and in every run) and runs Trainer.apply on every copy, so the replicas stay bit-identical without a broadcast"""

    def __init__(self, net, max_batch, T, devices, precision="f32"):
        from .network import _layers_array
        code = _train_precision_code(precision)
        self.h = None
        self.lib = _lib.load()
        self.net, self.T, self.max_batch = net, int(T), int(max_batch)
        self.devices = [int(d) for d in devices]
        self.R = len(self.devices)
        self._layers = _layers_array(net)
        dev = (C.c_int * max(self.R, 1))(*self.devices)
        self.h = self.lib.po_train_group_create(self._layers, len(net.layers), self.max_batch, self.T, dev, self.R)
        if not self.h:
            detail = self.lib.po_last_error()
            raise _lib.EngineError(_lib.E_ARG, "po_train_group_create", detail.decode() if detail else "")
        self.n_params = net.n_params()
        self.set_params(net.flat_weights())
        if code != _lib.TRAIN_PRECISIONS["f32"]:
            self.set_precision(precision)

    def set_precision(self, name):
        """Trainer.set_precision on every replica, or on none where it is refused"""
        _lib.check(self.lib.po_train_group_set_precision(self.h, _train_precision_code(name)), "po_train_group_set_precision")

    def close(self):
        if self.h:
            self.lib.po_train_group_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, flat):
        """load the parameters into every replica and reset Adam"""
        w = np.ascontiguousarray(flat, dtype=np.float32)
        _lib.check(self.lib.po_train_group_set_params(self.h, w.ctypes.data, w.size), "po_train_group_set_params")

    def get_params(self, replica=0):
        w = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self.lib.po_train_group_get_replica_params(self.h, int(replica), w.ctypes.data, w.size),
                   "po_train_group_get_replica_params")
        return w

    def network(self):
        """replica 0's parameters as a Network"""
        return self.net.with_flat(self.get_params())

    def _shares(self, micro):
        """the C layout of up to R micro-batches (None: that replica idles): counts, windows, label lengths, labels"""
        if len(micro) > self.R:
            raise ValueError("%d micro-batches for %d replicas" % (len(micro), self.R))
        micro = list(micro) + [None] * (self.R - len(micro))
        n = np.asarray([0 if mb is None else len(mb[0]) for mb in micro], dtype=np.int32)
        xs = [np.ascontiguousarray(mb[0], dtype=np.float32).reshape(len(mb[0]), -1) for mb in micro if mb is not None and len(mb[0])]
        x = np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros((1, self.T), dtype=np.float32)
        if x.shape[1] != self.T:
            raise ValueError("windows of %d samples, the group holds %d" % (x.shape[1], self.T))
        lens, lab = _flat_labels([l for mb in micro if mb is not None for l in mb[1]])
        if len(lens) != int(n.sum()):
            raise ValueError("%d label sequences for %d windows" % (len(lens), int(n.sum())))
        if not len(lens):
            lens = np.zeros(1, dtype=np.int32)
        return n, x, lens, lab

    def accumulate(self, micro, N, merge_repeated=False, stage_ms=None):
        """po_train_group_accumulate: micro is a list of up to R (windows, labels) pairs, micro-batch j for replica j (None:
        idle), all at once; each runs Trainer.accumulate with weight n_j / N, N the window count of the whole optimizer step.
        A micro-batch that is refused refuses the call for all.  Returns the micro-batches' per-window losses, a list"""
        n, x, lens, lab = self._shares(micro)
        weight = np.asarray([k / N for k in n], dtype=np.float32)
        loss = np.empty(max(int(n.sum()), 1), dtype=np.float32)
        ms = np.zeros((self.R, len(_lib.TRAIN_STAGES)), dtype=np.float32) if stage_ms is not None else None
        rc = self.lib.po_train_group_accumulate(self.h, x.ctypes.data, n.ctypes.data, lab.ctypes.data, lens.ctypes.data,
                                                1 if merge_repeated else 0, weight.ctypes.data, loss.ctypes.data,
                                                ms.ctypes.data if ms is not None else None)
        _lib.check(rc, "po_train_group_accumulate")
        if stage_ms is not None:
            stage_ms.append(ms)
        off = np.concatenate([[0], np.cumsum(n)])
        return [loss[off[j]:off[j + 1]].copy() for j in range(len(micro))]

    def reduce(self):
        """po_train_group_reduce: the all-reduce alone; the milliseconds between events on replica 0's stream"""
        ms = C.c_float()
        _lib.check(self.lib.po_train_group_reduce(self.h, C.byref(ms)), "po_train_group_reduce")
        return ms.value

    def apply(self, lr=1e-3, clip_norm=0.0, weight_decay=0.0, **adam):
        """po_train_group_apply: the all-reduce, then Trainer.apply on every replica; (grad_norm, applied) of replica 0"""
        a = dict(ADAM, **adam)
        norm, applied = C.c_double(), C.c_int()
        rc = self.lib.po_train_group_apply(self.h, float(lr), float(a["beta1"]), float(a["beta2"]), float(a["eps"]),
                                           float(weight_decay), float(clip_norm), C.byref(norm), C.byref(applied))
        _lib.check(rc, "po_train_group_apply")
        return norm.value, bool(applied.value)

    def get_accum(self, replica):
        g = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self.lib.po_train_group_get_accum(self.h, int(replica), g.ctypes.data, g.size), "po_train_group_get_accum")
        return g

    def set_accum(self, replica, g):
        """load one replica's accumulator (counts as one contribution): how a test plants a value in one share"""
        g = np.ascontiguousarray(g, dtype=np.float32)
        _lib.check(self.lib.po_train_group_set_accum(self.h, int(replica), g.ctypes.data, g.size), "po_train_group_set_accum")

    def get_state(self, replica=0):
        """(m, v, step) of a replica (0: what a checkpoint saves)"""
        m = np.empty(self.n_params, dtype=np.float32)
        v = np.empty(self.n_params, dtype=np.float32)
        step = C.c_int64()
        _lib.check(self.lib.po_train_group_get_replica_state(self.h, int(replica), m.ctypes.data, v.ctypes.data, m.size,
                                                             C.byref(step)), "po_train_group_get_replica_state")
        return m, v, int(step.value)

    def set_state(self, m, v, step):
        """load Adam's moments and step count into every replica (after set_params, which resets them)"""
        m = np.ascontiguousarray(m, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if m.size != v.size:
            raise ValueError("set_state: m has %d values, v %d" % (m.size, v.size))
        _lib.check(self.lib.po_train_group_set_state(self.h, m.ctypes.data, v.ctypes.data, m.size, int(step)), "po_train_group_set_state")

    def evaluate(self, micro, merge_repeated=False, loss=True, predictions=False):
        """po_train_group_eval: Trainer.evaluate of up to R (windows, labels) pairs, pair j on replica j, at the same time; a
        list of Trainer.evaluate's dicts"""
        n, x, lens, lab = self._shares(micro)
        tot = max(int(n.sum()), 1)
        edit, plen, st = (np.empty(tot, dtype=np.int32) for _ in range(3))
        ls = np.empty(tot, dtype=np.float32) if loss else None
        pred = np.empty((tot, self.T), dtype=np.uint8) if predictions else None
        rc = self.lib.po_train_group_eval(self.h, x.ctypes.data, n.ctypes.data, lab.ctypes.data, lens.ctypes.data,
                                          1 if merge_repeated else 0, ls.ctypes.data if loss else None, edit.ctypes.data,
                                          plen.ctypes.data, st.ctypes.data, pred.ctypes.data if predictions else None, None)
        _lib.check(rc, "po_train_group_eval")
        off = np.concatenate([[0], np.cumsum(n)])
        out = []
        for j in range(len(micro)):
            a, b = off[j], off[j + 1]
            d = {"edit": edit[a:b].copy(), "pred_len": plen[a:b].copy(), "status": st[a:b].copy()}
            if loss:
                d["loss"] = ls[a:b].copy()
            if predictions:
                d["pred"] = [pred[w, :plen[w]].copy() for w in range(a, b)]
            out.append(d)
        return out


def _split_labels(labels, row_lengths):
    off = np.concatenate([[0], np.cumsum(row_lengths)])
    return [labels[off[i]:off[i + 1]] for i in range(len(row_lengths))]


def _edit(a, b):
    from ..accuracy import alignment_summary
    return alignment_summary("".join("ACGT"[i] for i in a), "".join("ACGT"[i] for i in b))["edit_distance"]


def validation_error(net, batches, signal, labels):
    """the reference's validation_error: per held-out batch the mean over its windows of edit_distance(argmax of the
    softmax without class 4, truth) / len(truth) (repeats are not merged), then the mean over batches; windows with no
    labels are left out (TensorFlow would divide by zero)"""
    from .network import forward
    per_batch = []
    for b in batches:
        probs = forward(net, signal[b])
        best = np.argmax(probs, axis=2)
        d = [_edit(p[p < 4], labels[w]) / len(labels[w]) for p, w in zip(best, b) if len(labels[w])]
        if d:
            per_batch.append(np.mean(d))
    return float(np.mean(per_batch)) if per_batch else float("nan")


def validation_error_device(trainer, batches, signal, labels, stage_ms=None):
    """validation_error on the trainer's resident parameters (Trainer.evaluate: the forward pass, the argmax path and the
    edit distance stay on the device; no parameter leaves it): the same arithmetic in the same order and dtype, so the
    same float.  A window the device declines (status E_CAP) gets its distance on the host, from the downloaded path."""
    per_batch = []
    for b in batches:
        lab = [labels[w] for w in b]
        r = trainer.evaluate(signal[b], lab, loss=False, stage_ms=stage_ms)
        edit = [int(e) for e in r["edit"]]
        capped = [k for k in range(len(b)) if r["status"][k] != _lib.OK and len(lab[k])]
        if capped:
            pred = trainer.evaluate(signal[b], lab, loss=False, predictions=True)["pred"]
            for k in capped:
                edit[k] = _edit(pred[k], lab[k])
        d = [edit[k] / len(lab[k]) for k in range(len(b)) if len(lab[k])]
        if d:
            per_batch.append(np.mean(d))
    return float(np.mean(per_batch)) if per_batch else float("nan")


def validation_error_group(group, batches, signal, labels):
    """validation_error_device over a TrainerGroup: held batch i goes to replica i % R, R batches at a time; the edit
    distances are integers and the means are taken in batch order, so the figure is the single-device one exactly"""
    per_batch = []
    for i in range(0, len(batches), group.R):
        rnd = batches[i:i + group.R]
        labs = [[labels[w] for w in b] for b in rnd]
        res = group.evaluate([(signal[b], lab) for b, lab in zip(rnd, labs)], loss=False)
        preds = None
        for j, (b, lab, r) in enumerate(zip(rnd, labs, res)):
            edit = [int(e) for e in r["edit"]]
            capped = [k for k in range(len(b)) if r["status"][k] != _lib.OK and len(lab[k])]
            if capped:
                if preds is None:
                    preds = group.evaluate([(signal[x], l) for x, l in zip(rnd, labs)], loss=False, predictions=True)
                pred = preds[j]["pred"]
                for k in capped:
                    edit[k] = _edit(pred[k], lab[k])
            d = [edit[k] / len(lab[k]) for k in range(len(b)) if len(lab[k])]
            if d:
                per_batch.append(np.mean(d))
    return float(np.mean(per_batch)) if per_batch else float("nan")


def plan_steps(batches, gpus, accumulate):
    """the optimizer steps of a data-parallel run: a step is gpus · accumulate consecutive batches of the plan (the last
    step may be shorter); batch j of a step goes to replica j % gpus in round j // gpus, with weight len(batch) / windows of
    the step.  Returns, per step, its rounds: lists of (replica, batch, weight), replicas ascending from 0 (a shorter last
    round leaves the higher replicas idle)"""
    per = gpus * accumulate
    steps = []
    for i in range(0, len(batches), per):
        group = batches[i:i + per]
        n_step = sum(len(b) for b in group)
        steps.append([[(j % gpus, group[j], len(group[j]) / n_step) for j in range(k, min(k + gpus, len(group)))]
                      for k in range(0, len(group), gpus)])
    return steps


def _write_state(out_dir, names):
    with open(os.path.join(out_dir, "checkpoint"), "w") as fh:
        fh.write('model_checkpoint_path: "%s"\n' % names[-1])
        for n in names:
            fh.write('all_model_checkpoint_paths: "%s"\n' % n)


LR_SCHEDULES = ("constant", "linear", "cosine")


def lr_at(s, S, base, schedule="constant", warmup_steps=0, min_lr=0.0):
    """the learning rate of optimizer step s (the number of steps done before it) of a run of S: for s < warmup_steps
    base · (s + 1) / warmup_steps; after that, with x = (s − warmup_steps) / max(1, S − warmup_steps), `constant`: base,
    `linear`: base − (base − min_lr) · x, `cosine`: min_lr + (base − min_lr) · ½(1 + cos πx)"""
    if schedule not in LR_SCHEDULES:
        raise ValueError("lr schedule %r (one of %s)" % (schedule, ", ".join(LR_SCHEDULES)))
    if s < warmup_steps:
        return base * (s + 1) / warmup_steps
    x = (s - warmup_steps) / max(1, S - warmup_steps)
    if schedule == "linear":
        return base - (base - min_lr) * x
    if schedule == "cosine":
        return min_lr + (base - min_lr) * 0.5 * (1.0 + math.cos(math.pi * x))
    return base


RECIPE_DEFAULTS = dict(accumulate=1, clip_norm=0.0, weight_decay=0.0, lr_schedule="constant", warmup_steps=0, min_lr=0.0,
                       save_optimizer=False, resume_optimizer=False)


def _recipe(args):
    """the recipe's flags of `args` (a namespace may lack any of them: the default then), refused by name where they make
    no sense"""
    r = {k: getattr(args, k, d) for k, d in RECIPE_DEFAULTS.items()}
    if r["accumulate"] < 1:
        raise TrainError("train: --accumulate must be positive")
    for flag in ("clip_norm", "weight_decay", "warmup_steps", "min_lr"):
        if not r[flag] >= 0 or not math.isfinite(r[flag]):
            raise TrainError("train: --%s must be 0 or positive (and finite)" % flag)
    if r["lr_schedule"] not in LR_SCHEDULES:
        raise TrainError("train: --lr_schedule %s (one of %s)" % (r["lr_schedule"], ", ".join(LR_SCHEDULES)))
    if r["min_lr"] > args.learning_rate:
        raise TrainError("train: --min_lr %s is above --learning_rate %s" % (r["min_lr"], args.learning_rate))
    if r["resume_optimizer"] and not getattr(args, "restart", False):
        raise TrainError("train: --resume_optimizer needs --restart (it loads the .opt.npz beside that checkpoint)")
    return r


def optimizer_path(restart):
    """the .opt.npz `--save_optimizer` wrote beside the checkpoint that `--restart` resolves"""
    path = str(restart)
    if path.endswith(".npz"):
        return path[:-len(".npz")] + ".opt.npz"
    return ckpt.resolve_checkpoint(path) + ".opt.npz"


def load_optimizer(path, n_params):
    """(m, v, step, iteration) of an .opt.npz, checked against the model's weight count"""
    if not os.path.exists(path):
        raise TrainError("train: --resume_optimizer: %s is missing (write it with --save_optimizer)" % path)
    try:
        with np.load(path) as z:
            d = {k: z[k] for k in ("m", "v", "step", "iteration") if k in z.files}
    except (OSError, ValueError) as e:
        raise TrainError("train: cannot read the optimizer state %s: %s" % (path, e))
    if len(d) < 4:
        raise TrainError("train: %s is no optimizer file (it holds m, v, step and iteration)" % path)
    m, v, step, it = d["m"], d["v"], int(d["step"]), int(d["iteration"])
    if m.shape != (n_params,) or v.shape != (n_params,):
        raise TrainError("train: %s holds m and v of %d and %d values, the model has %d weights" % (path, m.size, v.size, n_params))
    if step < 0 or it < 0:
        raise TrainError("train: %s holds a negative step count" % path)
    return np.asarray(m, dtype=np.float32), np.asarray(v, dtype=np.float32), step, it


def _dp_devices(gpus):
    """the devices of a --gpus N run, 0 .. N - 1 (the command line repeats none); refused where fewer are visible"""
    nd = _lib.load(False).po_device_count()
    if gpus > nd:
        raise TrainError("train: --gpus %d, but %d device%s visible" % (gpus, nd, " is" if nd == 1 else "s are"))
    return list(range(gpus))


def _check_replicas(group, when):
    """the replicas of a group hold the same parameters, bit for bit: compared on the host, first against last"""
    a, b = group.get_params(0), group.get_params(group.R - 1)
    if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        raise TrainError("train: %s: replica 0 and replica %d hold different parameters (%d of %d values differ)" %
                         (when, group.R - 1, int(np.sum(a.view(np.uint32) != b.view(np.uint32))), a.size))


def _write_optimizer(path, tr, iteration):
    m, v, step = tr.get_state()
    np.savez(path, m=m, v=v, step=np.int64(step), iteration=np.int64(iteration))


def train(args):
    """`poreover train --data DATA.npz ...` (network.py:133-179); returns the output directory"""
    if args.num_neurons != ckpt.UNITS:
        raise TrainError("train: --num_neurons %d is not supported (the device kernels are built for %d GRU units)" %
                         (args.num_neurons, ckpt.UNITS))
    for flag in ("batch_size", "epochs", "save_every", "loss_every", "kernel_size", "filters"):
        if getattr(args, flag) < 1:
            raise TrainError("train: --%s must be positive" % flag)
    if args.kernel_size > ckpt.MAX_KERNEL:
        raise TrainError("train: --kernel_size %d is not supported (the device kernels take Conv1D kernels of 1 to %d taps)" %
                         (args.kernel_size, ckpt.MAX_KERNEL))
    if not 0.0 <= args.holdout < 1.0:
        raise TrainError("train: --holdout must be in [0, 1)")
    gemm_precision = getattr(args, "gemm_precision", "f32")
    if gemm_precision not in _lib.TRAIN_PRECISIONS:
        raise TrainError("train: --gemm_precision %s (one of %s)" % (gemm_precision, ", ".join(_lib.TRAIN_PRECISIONS)))
    recipe = _recipe(args)
    gpus = getattr(args, "gpus", 1)        # (a namespace may lack it: one device)
    if gpus < 1:
        raise TrainError("train: --gpus must be positive")
    devices = _dp_devices(gpus) if gpus > 1 else [0]
    # every flag of the recipe at its default, on one device: the loop below steps as it always has
    plain = recipe == RECIPE_DEFAULTS and gpus == 1
    signal, labels, row_lengths = load_data(args.data)
    N, T = signal.shape
    check_labels(labels, row_lengths, T, args.ctc_merge_repeated)
    config = ckpt.architecture(args.model, kernel_size=args.kernel_size, filters=args.filters)
    held, batches = plan_batches(N, args.batch_size, args.holdout, args.epochs, args.seed)
    if not batches:
        raise TrainError("train: %d windows leave no whole training batch of %d" % (N, args.batch_size))
    if args.restart:
        net = ckpt.load_network(args.restart, config)
    else:
        net = ckpt.load_network(init_weights(config, args.seed), config)
    opt_state = None
    if recipe["resume_optimizer"]:
        opt_state = load_optimizer(optimizer_path(args.restart), net.n_params())

    print("PoreOver train", file=sys.stderr)
    if gemm_precision != "f32":   # (train.log's header records the flag with the other arguments)
        print("GRU weight and input GEMMs: {} operands, f32 sums (--gemm_precision {})".format(gemm_precision, gemm_precision),
              file=sys.stderr)
    if gpus > 1:
        print("Data-parallel training on devices {} (--gpus {})".format(", ".join(str(d) for d in devices), gpus),
              file=sys.stderr)
    out_dir = "{}_{}_{}".format(args.model, args.name, datetime.datetime.now().strftime("%Y-%m-%d_%H-%M"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "train.log"), "w") as log:
        print("Command-line arguments:", file=log)
        for k, v in args.__dict__.items():
            if k != "func":
                print(k, "=", v, file=log)
        print("Setting aside {}% of data for validation: {} batches".format(args.holdout * 100, len(held)), file=log)
    with open(os.path.join(out_dir, "model.json"), "w") as fh:
        fh.write(json.dumps(config))

    lab_list = _split_labels(labels, row_lengths)
    saved = []
    # the recipe: an optimizer step is K consecutive batches of the plan (a shorter last group with its own
    # weights); t, --save_every and --loss_every count optimizer steps
    K = recipe["accumulate"]
    # with --gpus N > 1 it is N · K batches, batch j on replica j % N in round j // N (plan_steps)
    groups = [batches[i:i + K] for i in range(0, len(batches), K)] if gpus == 1 else plan_steps(batches, gpus, K)
    S = len(groups)
    with (Trainer(net, args.batch_size, T, precision=gemm_precision) if gpus == 1 else
          TrainerGroup(net, args.batch_size, T, devices, precision=gemm_precision)) as tr:
        done = 0                          # optimizer steps before this run: the schedule goes on from there
        if opt_state is not None:
            tr.set_state(opt_state[0], opt_state[1], opt_state[2])
            done = opt_state[3]
        for t, b in enumerate(batches if plain else groups):
            if plain:
                loss = tr.step(signal[b], [lab_list[i] for i in b], merge_repeated=args.ctc_merge_repeated,
                               lr=args.learning_rate)
            elif gpus > 1:
                n_group = sum(len(mb) for rnd in b for _, mb, _ in rnd)
                loss = np.concatenate([l for rnd in b for l in tr.accumulate(
                    [(signal[mb], [lab_list[i] for i in mb]) for _, mb, _ in rnd], n_group, merge_repeated=args.ctc_merge_repeated)])
                lr = lr_at(min(done + t, S - 1), S, args.learning_rate, recipe["lr_schedule"], recipe["warmup_steps"],
                           recipe["min_lr"])
                norm, applied = tr.apply(lr, clip_norm=recipe["clip_norm"], weight_decay=recipe["weight_decay"])
            else:
                n_group = sum(len(mb) for mb in b)
                loss = np.concatenate([tr.accumulate(signal[mb], [lab_list[i] for i in mb], len(mb) / n_group,
                                                     merge_repeated=args.ctc_merge_repeated) for mb in b])
                # (past the end of the schedule, which only a resumed run reaches, the rate keeps its last value)
                lr = lr_at(min(done + t, S - 1), S, args.learning_rate, recipe["lr_schedule"], recipe["warmup_steps"],
                           recipe["min_lr"])
                norm, applied = tr.apply(lr, clip_norm=recipe["clip_norm"], weight_decay=recipe["weight_decay"])
            mean = np.mean(loss, dtype=np.float32)
            if t % args.save_every == 0:
                if gpus > 1:
                    _check_replicas(tr, "iteration %d" % t)
                name = "checkpoint-%d" % len(saved)
                ckpt.write_weights(os.path.join(out_dir, name + ".npz"), tr.network())
                if recipe["save_optimizer"]:
                    _write_optimizer(os.path.join(out_dir, name + ".opt.npz"), tr, done + t + 1)
                saved.append(name)
                _write_state(out_dir, saved)
            if t % args.loss_every == 0:
                print("Iteration:{}\tLoss:{}".format(t, mean), file=sys.stderr)
            if not plain and recipe["clip_norm"] > 0 and t % args.loss_every == 0:
                print("Iteration:{}\tGradient norm:{}".format(t, norm), file=sys.stderr)
            if not plain and not applied:
                print("Iteration:{}\tSkipped: non-finite gradient".format(t), file=sys.stderr)
            if t % args.save_every == 0 and len(held) > 0:
                d = (validation_error_device if gpus == 1 else validation_error_group)(tr, held, signal, lab_list)
                print("Iteration:{}\tEdit distance (test):{}".format(t, d), file=sys.stderr)
        if gpus > 1:
            _check_replicas(tr, "the last iteration")
        ckpt.write_weights(os.path.join(out_dir, "final.npz"), tr.network())
        if recipe["save_optimizer"]:
            _write_optimizer(os.path.join(out_dir, "final.opt.npz"), tr, done + S)
    saved.append("final")
    _write_state(out_dir, saved)
    return out_dir
