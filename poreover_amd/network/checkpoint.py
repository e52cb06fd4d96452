"""Weights and architecture of the basecalling network, read without TensorFlow.

The reference loads a Keras model (`build_model(args).conv1_bigru3()` or `tf.keras.models.model_from_json(--model)`) and
`model.load_weights(checkpoint)` (network.py:181-203).  This module reads the same two inputs:

  * a TF2 object-based checkpoint, given as a prefix (`.../checkpoint-124`) or as a directory whose `checkpoint` text
    file names the latest prefix (what tf.train.latest_checkpoint does).  `<prefix>.index` is a leveldb-format table
    (uncompressed blocks) whose keys are tensor names and whose values are BundleEntryProto messages (dtype, shape,
    shard, offset, size, crc32c); `<prefix>.data-SSSSS-of-NNNNN` hold the bytes.  Every tensor's crc32c is checked.
  * or an `.npz` of the same tensor names (`python -m poreover_amd.network.convert CKPT out.npz` writes one);
  * a Keras JSON config (`--model`) or, without one, the default `conv1_bigru3` (network.py:30-36).

`load_network` turns both into a `Network`: a list of layers in the order the device runs them, each with f32 arrays
in Keras' own layouts (GRU kernel (Cin, 3H), recurrent kernel (H, 3H), bias (2, 3H) — gate order z, r, h; H units per
direction, one of UNITS_ACCEPTED and the same in every GRU layer —, Conv1D
kernel (K, Cin, F), Dense kernel (Cin, 5)).  Only what the four `build_model` architectures use is accepted; anything
else raises NetworkError naming it."""
import json
import os
import re
import struct

import numpy as np

__all__ = ["NetworkError", "Layer", "Network", "read_index", "read_checkpoint", "read_weights", "resolve_checkpoint",
           "parse_model_json", "default_model_config", "UNITS", "UNITS_ACCEPTED", "load_network", "synthetic_weights", "ARCHITECTURES", "architecture",
           "write_weights", "crc32c"]

UNITS = 128          # the default GRU width (build_model's num_neurons default)
UNITS_ACCEPTED = (16, 32, 48, 64, 80, 96, 112, 128)   # units per direction the device kernels are built for (one wave
                     # per 16 units, at most 8 waves: csrc/po_call_kernels.h); one width for every GRU layer of a model
NUM_LABELS = 5       # A, C, G, T, blank
MAX_KERNEL = 64      # the longest Conv1D kernel the device takes (check_model in csrc/po_call_kernels.h); any filters >= 1


class NetworkError(ValueError):
    pass


# ---- crc32c (Castagnoli), as TF masks it in BundleEntryProto --------------------------------------------------------
def _crc_tables():
    poly = 0x82F63B78
    t0 = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ poly if c & 1 else c >> 1
        t0[i] = c
    tabs = [t0]
    for _ in range(7):      # slicing-by-8
        prev = tabs[-1]
        tabs.append((prev >> 8) ^ t0[prev & 0xFF])
    return [t.tolist() for t in tabs]


_CRC_T = None


def crc32c(data):
    global _CRC_T
    if _CRC_T is None:
        _CRC_T = _crc_tables()
    t0, t1, t2, t3, t4, t5, t6, t7 = _CRC_T
    crc = 0xFFFFFFFF
    b = bytes(data)
    n8 = len(b) // 8 * 8
    for lo, hi in struct.iter_unpack("<II", b[:n8]):
        lo ^= crc
        crc = (t7[lo & 0xFF] ^ t6[(lo >> 8) & 0xFF] ^ t5[(lo >> 16) & 0xFF] ^ t4[lo >> 24] ^
               t3[hi & 0xFF] ^ t2[(hi >> 8) & 0xFF] ^ t1[(hi >> 16) & 0xFF] ^ t0[hi >> 24])
    for x in b[n8:]:
        crc = t0[(crc ^ x) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def _unmask(m):
    rot = (m - 0xA282EAD8) & 0xFFFFFFFF
    return ((rot >> 17) | (rot << 15)) & 0xFFFFFFFF


# ---- protobuf / leveldb table --------------------------------------------------------------------------------------
def _varint(b, pos):
    x = shift = 0
    while True:
        c = b[pos]
        pos += 1
        x |= (c & 0x7F) << shift
        if c < 0x80:
            return x, pos
        shift += 7


def _proto_fields(b):
    """(field number, wire type, value) of one protobuf message: varints as int, length-delimited as bytes"""
    pos, out = 0, []
    while pos < len(b):
        key, pos = _varint(b, pos)
        fn, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(b, pos)
        elif wt == 1:
            v = struct.unpack_from("<Q", b, pos)[0]; pos += 8
        elif wt == 2:
            n, pos = _varint(b, pos)
            v = bytes(b[pos:pos + n]); pos += n
        elif wt == 5:
            v = struct.unpack_from("<I", b, pos)[0]; pos += 4
        else:
            raise NetworkError("checkpoint index: protobuf wire type %d" % wt)
        out.append((fn, wt, v))
    return out


_DTYPES = {1: np.float32, 2: np.float64, 3: np.int32, 4: np.uint8, 5: np.int16, 6: np.int8, 9: np.int64, 10: np.bool_,
           19: np.float16}
_DT_STRING = 7


def _block_entries(buf, off, size):
    if buf[off + size] != 0:
        raise NetworkError("checkpoint index: compressed table block (type %d)" % buf[off + size])
    blk = buf[off:off + size]
    nrest, = struct.unpack_from("<I", blk, len(blk) - 4)
    end = len(blk) - 4 - 4 * nrest
    pos, key, out = 0, b"", []
    while pos < end:
        shared, pos = _varint(blk, pos)
        nons, pos = _varint(blk, pos)
        vlen, pos = _varint(blk, pos)
        key = key[:shared] + blk[pos:pos + nons]
        pos += nons
        out.append((key, blk[pos:pos + vlen]))
        pos += vlen
    return out


def read_index(path):
    """{tensor name: dict(dtype, shape, shard, offset, size, crc32c)} of a `.index` file, and the number of shards"""
    with open(path, "rb") as fh:
        buf = fh.read()
    if len(buf) < 48 or struct.unpack_from("<Q", buf, len(buf) - 8)[0] != 0xDB4775248B80FB57:
        raise NetworkError("%s is not a TF checkpoint index (leveldb table magic)" % path)
    foot = buf[len(buf) - 48:]
    _mo, p = _varint(foot, 0)
    _ms, p = _varint(foot, p)
    io, p = _varint(foot, p)
    isz, p = _varint(foot, p)
    entries, nshards = {}, 1
    for _k, handle in _block_entries(buf, io, isz):
        bo, q = _varint(handle, 0)
        bs, q = _varint(handle, q)
        for key, val in _block_entries(buf, bo, bs):
            if key == b"":            # BundleHeaderProto
                for fn, _wt, v in _proto_fields(val):
                    if fn == 1:
                        nshards = v
                    elif fn == 2 and v != 0:
                        raise NetworkError("checkpoint written big-endian")
                continue
            e = dict(dtype=1, shape=(), shard=0, offset=0, size=0, crc32c=None)
            for fn, _wt, v in _proto_fields(val):
                if fn == 1:
                    e["dtype"] = v
                elif fn == 2:
                    dims = []
                    for f2, _w2, v2 in _proto_fields(v):
                        if f2 == 2:
                            dims.append(next((s for f3, _w3, s in _proto_fields(v2) if f3 == 1), 0))
                    e["shape"] = tuple(dims)
                elif fn == 3:
                    e["shard"] = v
                elif fn == 4:
                    e["offset"] = v
                elif fn == 5:
                    e["size"] = v
                elif fn == 6:
                    e["crc32c"] = v
                elif fn == 7:
                    raise NetworkError("checkpoint index: partitioned (sliced) tensor %s" % key.decode())
            entries[key.decode()] = e
    return entries, nshards


def resolve_checkpoint(path):
    """a checkpoint prefix from a prefix, a `.index` path or a directory with a `checkpoint` file"""
    if os.path.isdir(path):
        state = os.path.join(path, "checkpoint")
        if not os.path.exists(state):
            raise NetworkError("%s is a directory without a `checkpoint` file" % path)
        m = re.search(r'^model_checkpoint_path:\s*"(.*)"\s*$', open(state).read(), re.M)
        if not m:
            raise NetworkError("%s names no model_checkpoint_path" % state)
        p = m.group(1)
        return p if os.path.isabs(p) else os.path.join(path, p)
    if path.endswith(".index"):
        return path[:-len(".index")]
    return path


def read_checkpoint(prefix, names=None, verify=True):
    """{name: array} of the numeric tensors of the checkpoint at `prefix` (or only `names`), crc32c-checked"""
    prefix = resolve_checkpoint(prefix)
    if not os.path.exists(prefix + ".index"):
        raise NetworkError("no checkpoint at %s (%s.index is missing)" % (prefix, prefix))
    entries, nshards = read_index(prefix + ".index")
    shards = {}
    out = {}
    for name, e in entries.items():
        if e["dtype"] == _DT_STRING or (names is not None and name not in names):
            continue
        if e["dtype"] not in _DTYPES:
            raise NetworkError("tensor %s: dtype %d" % (name, e["dtype"]))
        sh = e["shard"]
        if sh not in shards:
            fn = "%s.data-%05d-of-%05d" % (prefix, sh, nshards)
            if not os.path.exists(fn):
                raise NetworkError("checkpoint shard %s is missing" % fn)
            with open(fn, "rb") as fh:
                shards[sh] = fh.read()
        raw = shards[sh][e["offset"]:e["offset"] + e["size"]]
        if len(raw) != e["size"]:
            raise NetworkError("tensor %s runs past the end of its shard" % name)
        if verify and e["crc32c"] is not None and crc32c(raw) != _unmask(e["crc32c"]):
            raise NetworkError("tensor %s: crc32c mismatch (corrupt checkpoint)" % name)
        out[name] = np.frombuffer(raw, dtype=np.dtype(_DTYPES[e["dtype"]]).newbyteorder("<")).reshape(e["shape"]).copy()
    return out


def read_weights(path):
    """tensors from a checkpoint (prefix / directory) or an .npz of the same names; a resolved prefix without a `.index`
    whose `<prefix>.npz` exists (what `train` writes) is read from that"""
    path = str(path)
    if not path.endswith(".npz"):
        prefix = resolve_checkpoint(path)
        if not os.path.exists(prefix + ".index") and os.path.exists(prefix + ".npz"):
            path = prefix + ".npz"
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    return read_checkpoint(path)


def write_weights(path, net):
    """an .npz of `net`'s tensors under the checkpoint's tensor names (what read_weights / load_network read back)"""
    v = "/.ATTRIBUTES/VARIABLE_VALUE"
    out = {}
    for l in net.layers:
        for name, t in zip(l.names, l.tensors):
            out[name + v] = np.asarray(t, dtype=np.float32)
    np.savez(path, **out)
    return path if str(path).endswith(".npz") else str(path) + ".npz"


# ---- architecture ---------------------------------------------------------------------------------------------------
class Layer:
    """one layer as the device runs it: kind in conv | bigru | gru | gru_back | dense, and its f32 tensors in Keras'
    layouts (`tensors`: conv / dense [kernel, bias]; GRU: per direction [kernel, recurrent_kernel, bias])"""

    def __init__(self, kind, cin, cout, kernel=0, tensors=None, names=None):
        self.kind, self.cin, self.cout, self.kernel = kind, cin, cout, kernel
        self.tensors = tensors or []
        self.names = names or []

    def __repr__(self):
        return "Layer(%s, %d -> %d%s)" % (self.kind, self.cin, self.cout, ", k=%d" % self.kernel if self.kernel else "")


class Network:
    def __init__(self, layers):
        self.layers = layers

    @property
    def kinds(self):
        return [l.kind for l in self.layers]

    def flat_weights(self):
        """every tensor back to back in the order include/poreover_hip.h documents for po_call_batch"""
        return np.concatenate([np.ascontiguousarray(t, dtype=np.float32).ravel() for l in self.layers for t in l.tensors])

    def n_params(self):
        return int(sum(t.size for l in self.layers for t in l.tensors))

    def with_flat(self, flat):
        """a Network of the same layers whose tensors are taken, in order, from a flat vector (flat_weights' layout)"""
        flat = np.asarray(flat, dtype=np.float32)
        if flat.size != self.n_params():
            raise NetworkError("%d weights given, the model has %d" % (flat.size, self.n_params()))
        layers, k = [], 0
        for l in self.layers:
            ts = []
            for t in l.tensors:
                ts.append(flat[k:k + t.size].reshape(t.shape).copy())
                k += t.size
            layers.append(Layer(l.kind, l.cin, l.cout, l.kernel, ts, list(l.names)))
        return Network(layers)


def _conv(k=9, filters=256, first=False, input_size=1000):
    cfg = {"name": "conv1d", "trainable": True, "dtype": "float32", "filters": filters, "kernel_size": [k], "strides": [1],
           "padding": "same", "data_format": "channels_last", "dilation_rate": [1], "groups": 1, "activation": "relu",
           "use_bias": True}
    if first:
        cfg["batch_input_shape"] = [None, input_size, 1]
    return {"class_name": "Conv1D", "config": cfg}


def _gru(units=128, go_backwards=False):
    return {"class_name": "GRU", "config": {"name": "gru", "trainable": True, "dtype": "float32", "return_sequences": True,
                                            "return_state": False, "go_backwards": go_backwards, "stateful": False,
                                            "unroll": False, "time_major": False, "units": units, "activation": "tanh",
                                            "recurrent_activation": "sigmoid", "use_bias": True, "dropout": 0.0,
                                            "recurrent_dropout": 0.0, "implementation": 2, "reset_after": True}}


def _bigru(units=128, first=False, input_size=1000):
    cfg = {"name": "bidirectional", "trainable": True, "dtype": "float32", "layer": _gru(units), "merge_mode": "concat"}
    if first:
        cfg["batch_input_shape"] = [None, input_size, 1]
    return {"class_name": "Bidirectional", "config": cfg}


def _dense(units=NUM_LABELS):
    return {"class_name": "Dense", "config": {"name": "dense", "trainable": True, "dtype": "float32", "units": units,
                                              "activation": "linear", "use_bias": True}}


def _sequential(layers):
    return {"class_name": "Sequential", "config": {"name": "sequential", "layers": layers}}


# the four models of build_model (network.py:15-55), as Keras serialises them (model.to_json())
ARCHITECTURES = {
    "bigru3": lambda: _sequential([_bigru(first=True), _bigru(), _bigru(), _dense()]),
    "conv1_bigru3": lambda: _sequential([_conv(first=True), _bigru(), _bigru(), _bigru(), _dense()]),
    "conv2_bigru3": lambda: _sequential([_conv(first=True), _conv(), _bigru(), _bigru(), _bigru(), _dense()]),
    "conv1_gru5": lambda: _sequential([_conv(first=True), _gru(), _gru(go_backwards=True), _gru(), _gru(go_backwards=True),
                                       _gru(), _dense()]),
}


def architecture(name, kernel_size=9, filters=256, units=UNITS):
    """the Keras config of build_model(args).<name>() with its --kernel_size, --filters and --num_neurons
    (network.py:14-55)"""
    if name not in ARCHITECTURES:
        _refuse("architecture %s" % name)
    conv = lambda first=False: _conv(k=kernel_size, filters=filters, first=first)
    gru = lambda back=False: _gru(units, go_backwards=back)
    bigru = lambda first=False: _bigru(units, first=first)
    return {
        "bigru3": lambda: _sequential([bigru(True), bigru(), bigru(), _dense()]),
        "conv1_bigru3": lambda: _sequential([conv(True), bigru(), bigru(), bigru(), _dense()]),
        "conv2_bigru3": lambda: _sequential([conv(True), conv(), bigru(), bigru(), bigru(), _dense()]),
        "conv1_gru5": lambda: _sequential([conv(True), gru(), gru(True), gru(), gru(True), gru(), _dense()]),
    }[name]()


def default_model_config():
    """what the reference builds without --model: build_model(args).conv1_bigru3() (network.py:184-186)"""
    return ARCHITECTURES["conv1_bigru3"]()


def _refuse(what):
    raise NetworkError("unsupported model: %s (supported: the build_model architectures %s)" % (what, ", ".join(ARCHITECTURES)))


_ACCEPTED_TEXT = "the device kernels are built for %s units per direction, one width for every GRU layer" % \
                 ", ".join(str(u) for u in UNITS_ACCEPTED)


def _check_gru(c, where, model_units=None):
    """refuse what the device does not run; returns the layer's units.  model_units: the width of the model's earlier GRU
    layers (None for the first)"""
    units = c.get("units")
    if isinstance(units, bool) or not isinstance(units, int) or units not in UNITS_ACCEPTED:
        _refuse("%s has %s units (%s)" % (where, units, _ACCEPTED_TEXT))
    if model_units is not None and units != model_units:
        _refuse("%s has %d units, an earlier GRU layer has %d (%s)" % (where, units, model_units, _ACCEPTED_TEXT))
    if not c.get("reset_after", False):
        _refuse("%s has reset_after=False" % where)
    if c.get("activation", "tanh") != "tanh" or c.get("recurrent_activation", "sigmoid") != "sigmoid":
        _refuse("%s activations %s / %s (only tanh / sigmoid)" % (where, c.get("activation"), c.get("recurrent_activation")))
    if not c.get("use_bias", True):
        _refuse("%s without bias" % where)
    if not c.get("return_sequences", False) or c.get("return_state", False) or c.get("stateful", False):
        _refuse("%s must return sequences, without state" % where)
    if c.get("time_major", False):
        _refuse("%s is time-major" % where)
    return units


def parse_model_json(config):
    """[(kind, spec)] of a Keras Sequential model config (a JSON string, a parsed dict or a path to a JSON file);
    kinds: conv (kernel, filters) | bigru (units) | gru (units) | gru_back (units) | dense; units: per direction, one of
    UNITS_ACCEPTED and the same for every GRU layer"""
    if isinstance(config, str):
        config = json.loads(open(config).read() if os.path.exists(config) else config)
    if config.get("class_name") != "Sequential":
        _refuse("model class %s (only Sequential)" % config.get("class_name"))
    layers = config["config"]["layers"] if isinstance(config["config"], dict) else config["config"]
    out, units = [], None
    for i, ly in enumerate(layers):
        cls, c = ly.get("class_name"), ly.get("config", {})
        where = "layer %d (%s)" % (i, cls)
        if cls == "InputLayer":
            continue
        if cls == "Conv1D":
            ks = c.get("kernel_size", [1])
            ks = ks[0] if isinstance(ks, (list, tuple)) else ks
            st = c.get("strides", [1])
            st = st[0] if isinstance(st, (list, tuple)) else st
            dl = c.get("dilation_rate", [1])
            dl = dl[0] if isinstance(dl, (list, tuple)) else dl
            if st != 1:
                _refuse("%s has strides %s (only 1)" % (where, st))
            if dl != 1 or c.get("groups", 1) != 1:
                _refuse("%s is dilated or grouped" % where)
            if c.get("padding") != "same" or c.get("activation") != "relu" or not c.get("use_bias", True):
                _refuse("%s must be padding='same', activation='relu', with bias" % where)
            if c.get("data_format", "channels_last") != "channels_last":
                _refuse("%s is channels_first" % where)
            out.append(("conv", {"kernel": int(ks), "filters": int(c["filters"])}))
        elif cls == "Bidirectional":
            inner = c.get("layer", {})
            if inner.get("class_name") != "GRU":
                _refuse("%s wraps %s (only GRU)" % (where, inner.get("class_name")))
            if c.get("merge_mode", "concat") != "concat":
                _refuse("%s merge_mode %s (only concat)" % (where, c.get("merge_mode")))
            ic = inner.get("config", {})
            units = _check_gru(ic, where, units)
            if ic.get("go_backwards", False):
                _refuse("%s wraps a go_backwards GRU" % where)
            if "backward_layer" in c:
                _check_gru(c["backward_layer"].get("config", {}), where + " backward layer", units)
            out.append(("bigru", {"units": units}))
        elif cls == "GRU":
            units = _check_gru(c, where, units)
            out.append(("gru_back" if c.get("go_backwards", False) else "gru", {"units": units}))
        elif cls == "Dense":
            if c.get("units") != NUM_LABELS or c.get("activation", "linear") not in ("linear", None) or not c.get("use_bias", True):
                _refuse("%s must be Dense(%d) with bias and no activation" % (where, NUM_LABELS))
            if i != len(layers) - 1:
                _refuse("%s: Dense is only supported as the last layer" % where)
            out.append(("dense", {}))
        else:
            _refuse("%s: layer type %s" % (where, cls))
    if not out or out[-1][0] != "dense":
        _refuse("the model must end in Dense(%d)" % NUM_LABELS)
    return out


def _pick(w, *names):
    for n in names:
        if n in w:
            return np.asarray(w[n], dtype=np.float32)
    raise NetworkError("the weights hold no tensor %s" % names[0])


def load_network(weights, model=None):
    """Network from weights (a {name: array} dict, a checkpoint prefix / directory or an .npz) and an architecture
    (Keras JSON path / string / dict; None: conv1_bigru3).  Shapes are checked against the architecture."""
    spec = parse_model_json(model if model is not None else default_model_config())
    w = weights if isinstance(weights, dict) else read_weights(weights)
    layers, cin = [], 1
    for i, (kind, s) in enumerate(spec):
        p = "layer_with_weights-%d/" % i
        v = "/.ATTRIBUTES/VARIABLE_VALUE"
        if kind == "conv":
            k, b = _pick(w, p + "kernel" + v), _pick(w, p + "bias" + v)
            want = (s["kernel"], cin, s["filters"])
            if k.shape != want or b.shape != (s["filters"],):
                raise NetworkError("%skernel has shape %s, the model needs %s" % (p, k.shape, want))
            layers.append(Layer("conv", cin, s["filters"], s["kernel"], [k, b], [p + "kernel", p + "bias"]))
            cin = s["filters"]
        elif kind == "dense":
            k, b = _pick(w, p + "kernel" + v), _pick(w, p + "bias" + v)
            if k.shape != (cin, NUM_LABELS) or b.shape != (NUM_LABELS,):
                raise NetworkError("%skernel has shape %s, the model needs %s" % (p, k.shape, (cin, NUM_LABELS)))
            layers.append(Layer("dense", cin, NUM_LABELS, 0, [k, b], [p + "kernel", p + "bias"]))
        else:
            dirs = ["forward_layer/", "backward_layer/"] if kind == "bigru" else [""]
            H = s["units"]
            ts, names = [], []
            for d in dirs:
                q = p + d
                k = _pick(w, q + "cell/kernel" + v, q + "kernel" + v)
                u = _pick(w, q + "cell/recurrent_kernel" + v, q + "recurrent_kernel" + v)
                b = _pick(w, q + "cell/bias" + v, q + "bias" + v)
                if k.shape != (cin, 3 * H) or u.shape != (H, 3 * H) or b.shape != (2, 3 * H):
                    raise NetworkError("%s GRU tensors have shapes %s %s %s, the model needs %s %s %s" % (
                        q, k.shape, u.shape, b.shape, (cin, 3 * H), (H, 3 * H), (2, 3 * H)))
                ts += [k, u, b]
                names += [q + "cell/kernel", q + "cell/recurrent_kernel", q + "cell/bias"]
            cout = H * len(dirs)
            layers.append(Layer(kind, cin, cout, 0, ts, names))
            cin = cout
    return Network(layers)


def synthetic_weights(model=None, stats=None, seed=0):
    """{name: array} of seeded random weights for an architecture, drawn per tensor as N(mean, std) with the statistics
    of `stats` ({role: [mean, std]}, roles conv0 / gru / dense + "/kernel", "/bias", "/recurrent_kernel"; e.g.
    tests/golden/call_weight_stats.json) — or, for a role it lacks, N(0, 1 / fan_in)"""
    spec = parse_model_json(model if model is not None else default_model_config())
    rng = np.random.default_rng(seed)
    out, cin = {}, 1
    v = "/.ATTRIBUTES/VARIABLE_VALUE"

    def draw(name, shape, role, fan_in):
        m, s = (stats or {}).get(role, (0.0, 1.0 / np.sqrt(fan_in)))
        out[name + v] = (m + s * rng.standard_normal(shape)).astype(np.float32)

    for i, (kind, s) in enumerate(spec):
        p = "layer_with_weights-%d/" % i
        if kind == "conv":
            role = "conv0" if cin == 1 else "conv_deep"      # the shipped model has one Conv1D, on the 1-channel signal
            draw(p + "kernel", (s["kernel"], cin, s["filters"]), role + "/kernel", s["kernel"] * cin)
            draw(p + "bias", (s["filters"],), role + "/bias", s["kernel"] * cin)
            cin = s["filters"]
        elif kind == "dense":
            draw(p + "kernel", (cin, NUM_LABELS), "dense/kernel", cin)
            draw(p + "bias", (NUM_LABELS,), "dense/bias", cin)
        else:
            dirs = ["forward_layer/", "backward_layer/"] if kind == "bigru" else [""]
            H = s["units"]
            for d in dirs:
                q = p + d + "cell/"
                draw(q + "kernel", (cin, 3 * H), "gru/kernel" if cin > 1 else "gru_signal/kernel", cin)
                draw(q + "recurrent_kernel", (H, 3 * H), "gru/recurrent_kernel", H)
                draw(q + "bias", (2, 3 * H), "gru/bias", H)
            cin = H * len(dirs)
    return out
