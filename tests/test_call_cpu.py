"""`call` on the host: FAST5 attributes (hdf5_lite), signal filter and scaling, windowing, the checkpoint index, the Keras
JSON architectures and the refusals; with the reference checkout present, its real checkpoint through the float64
restatement (tests/_call_oracle.py) on the complementary pair read_316 / read_318."""
import glob
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FAST5_DIR = os.path.join(GOLDEN, "fast5")
REFERENCE = os.environ.get("POREOVER_REFERENCE", "/root/reference")
REF_CKPT = os.path.join(REFERENCE, "data", "model", "checkpoint-124")


def _fast5(tag):
    return glob.glob(os.path.join(FAST5_DIR, "*%s*" % tag))[0]


FILES = ["read_316", "read_318", "read.fast5"]


@pytest.mark.parametrize("tag", FILES)
def test_fast5_attributes(tag):
    from poreover_amd.decoding import hdf5_lite
    h = hdf5_lite.File(_fast5(tag))
    rs = h["/Raw/Reads"].keys()
    assert len(rs) == 1
    r = h["/Raw/Reads/" + rs[0]]
    sig = np.array(h["/Raw/Reads/" + rs[0] + "/Signal"])
    assert int(r.attrs["duration"]) == len(sig)
    rid = r.attrs["read_id"]
    assert isinstance(rid, bytes) and len(rid.decode()) == 36 and rid.decode().count("-") == 4
    ch = h["UniqueGlobalKey"]["channel_id"].attrs
    assert float(ch["digitisation"]) == 8192.0 and float(ch["sampling_rate"]) == 4000.0
    assert 1000 < float(ch["range"]) < 2000 and float(ch["offset"]) in (3.0, 15.0)
    assert set(ch.keys()) >= {"digitisation", "range", "offset", "sampling_rate", "channel_number"}
    assert sig.dtype == np.int16 and "read_id" in r.attrs and "nope" not in r.attrs
    with pytest.raises(KeyError):
        r.attrs["nope"]


def test_fast5_attributes_known_values():
    from poreover_amd.decoding import hdf5_lite
    r = hdf5_lite.File(_fast5("read_316"))["/Raw/Reads/Read_316"]
    assert r.attrs["read_id"] == b"9ffff59d-504a-433e-b607-f874da18e057"
    assert int(r.attrs["read_number"]) == 316 and int(r.attrs["start_time"]) == 4286796
    assert abs(float(r.attrs["median_before"]) - 219.1007537841797) < 1e-12
    # a dataset's attributes (none here) and the existing trace reader are unchanged
    assert len(hdf5_lite.File(_fast5("read_316"))["/Raw/Reads/Read_316/Signal"].attrs) == 0


def test_vlen_string_attribute_parses():
    """an attribute message of version 3 holding a variable-length string (global heap), built by hand"""
    import struct
    from poreover_amd.decoding import hdf5_lite
    text = b"abc-123"
    # global heap collection at address 8: one object
    obj = struct.pack("<HH4xQ", 1, 1, len(text)) + text + b"\0" * (8 - len(text) % 8)
    col = b"GCOL" + bytes([1, 0, 0, 0]) + struct.pack("<Q", 16 + len(obj) + 16) + obj + b"\0" * 16

    class F:
        buf = bytes(8) + col
        base = 0

    dt = bytes([0x19, 0x01, 0x00, 0x00]) + struct.pack("<I", 16) + bytes([0x10, 0, 0, 0]) + struct.pack("<I", 1)
    ds = bytes([2, 0, 0, 0])                                      # version-2 scalar dataspace
    name = b"read_id\0"
    data = struct.pack("<IQI", len(text), 8, 1)
    msg = bytes([3, 0]) + struct.pack("<HHH", len(name), len(dt), len(ds)) + b"\0" + name + dt + ds + data

    class O:
        def find(self, t):
            return [(0x000C, 0, msg)] if t == 0x000C else []

    a = hdf5_lite.Attributes(F(), O(), "/x")
    assert a["read_id"] == "abc-123"


@pytest.mark.parametrize("scaling", ["standard", "current", "median", "rescale", "raw"])
@pytest.mark.parametrize("tag", FILES)
def test_parse_fast5_filter_and_scaling(tag, scaling):
    from poreover_amd.decoding import hdf5_lite
    from poreover_amd.network import parse_fast5
    h = hdf5_lite.File(_fast5(tag))
    rs = h["/Raw/Reads"].keys()[0]
    raw = np.array(h["/Raw/Reads/" + rs + "/Signal"])
    ch = h["UniqueGlobalKey"]["channel_id"].attrs
    keep = raw[(raw > 200) & (raw < 800)]
    rid, sig = parse_fast5(_fast5(tag), scaling=scaling)
    assert rid == h["/Raw/Reads/" + rs].attrs["read_id"]
    assert len(sig) == len(keep)
    x = keep.astype(np.float64)
    want = {"standard": (x - x.mean()) / x.std(),
            "current": (x + ch["offset"]) / (ch["digitisation"] / ch["range"]),
            "median": x / np.median(x),
            "rescale": (x - x.mean()) / (x.max() - x.min()),
            "raw": keep}[scaling]
    np.testing.assert_allclose(sig, want, rtol=1e-12, atol=1e-12)
    if scaling == "standard":
        assert abs(sig.mean()) < 1e-9 and abs(sig.std() - 1) < 1e-9      # population std (np.std)


def test_read_fast5_drops_out_of_range_samples():
    from poreover_amd.decoding import hdf5_lite
    from poreover_amd.network import parse_fast5
    h = hdf5_lite.File(_fast5("read.fast5"))
    raw = np.array(h["/Raw/Reads/Read_70/Signal"])
    assert len(raw) - len(parse_fast5(_fast5("read.fast5"))[1]) == 296


@pytest.mark.parametrize("window", [1000, 400, 333])
@pytest.mark.parametrize("tag", FILES)
def test_batch_input_pads_and_trims(tag, window):
    from poreover_amd.network import batch_input, parse_fast5
    sig = parse_fast5(_fast5(tag))[1]
    wins, frames = batch_input(sig, window)
    assert frames == len(sig)
    assert wins.shape == (-(-len(sig) // window), window) and wins.dtype == np.float32
    flat = wins.ravel()
    np.testing.assert_array_equal(flat[:len(sig)], sig.astype(np.float32))
    assert not flat[len(sig):].any()
    # a read shorter than one window is one padded window
    w1, f1 = batch_input(sig[:10], window)
    assert w1.shape == (1, window) and f1 == 10


def test_checkpoint_index_committed():
    from poreover_amd.network import checkpoint as C
    entries, nshards = C.read_index(os.path.join(GOLDEN, "checkpoint-124.index"))
    assert nshards == 2
    num = {k: e for k, e in entries.items() if e["dtype"] == 1}
    assert len(num) == 22 and all(k.startswith("layer_with_weights-") for k in num)
    assert sum(int(np.prod(e["shape"])) for e in num.values()) == 893189
    assert sum(e["size"] for e in num.values()) == 3572756
    assert {e["shard"] for e in num.values()} == {1}
    assert num["layer_with_weights-1/forward_layer/cell/bias/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == (2, 384)
    assert num["layer_with_weights-0/kernel/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == (9, 1, 256)
    stats = json.load(open(os.path.join(GOLDEN, "call_weight_stats.json")))
    assert stats["n_params"] == 893189 and len(stats["tensors"]) == 22
    for k, (_m, _s, shape) in stats["tensors"].items():
        assert tuple(shape) == num[k]["shape"]


def test_crc32c_known_vectors():
    from poreover_amd.network.checkpoint import crc32c
    assert crc32c(b"123456789") == 0xE3069283
    assert crc32c(b"") == 0
    assert crc32c(bytes(32)) == 0x8A9136AA


def test_resolve_checkpoint_directory(tmp_path):
    from poreover_amd.network.checkpoint import resolve_checkpoint
    (tmp_path / "checkpoint").write_text('model_checkpoint_path: "checkpoint-124"\nall_model_checkpoint_paths: "checkpoint-100"\n')
    assert resolve_checkpoint(str(tmp_path)) == str(tmp_path / "checkpoint-124")
    assert resolve_checkpoint("/x/checkpoint-7.index") == "/x/checkpoint-7"
    assert resolve_checkpoint("/x/checkpoint-7") == "/x/checkpoint-7"


def test_corrupt_checkpoint_refused(tmp_path):
    """the committed index over a shard of the wrong bytes: the crc32c check refuses it, the unchecked read has the shape"""
    import shutil
    from poreover_amd.network import checkpoint as C
    idx = os.path.join(GOLDEN, "checkpoint-124.index")
    entries, _ = C.read_index(idx)
    name = "layer_with_weights-4/bias/.ATTRIBUTES/VARIABLE_VALUE"
    e = entries[name]
    shard = bytearray(3572756)
    prefix = str(tmp_path / "checkpoint-124")
    shutil.copy(idx, prefix + ".index")
    open(prefix + ".data-00001-of-00002", "wb").write(bytes(shard))
    with pytest.raises(C.NetworkError, match="crc32c"):
        C.read_checkpoint(prefix, names={name})
    assert C.read_checkpoint(prefix, names={name}, verify=False)[name].shape == e["shape"]


@pytest.mark.parametrize("arch,kinds,n_params", [
    ("bigru3", ["bigru", "bigru", "bigru", "dense"], 694789),
    ("conv1_bigru3", ["conv", "bigru", "bigru", "bigru", "dense"], 893189),
    ("conv2_bigru3", ["conv", "conv", "bigru", "bigru", "bigru", "dense"], 1483269),
    ("conv1_gru5", ["conv", "gru", "gru_back", "gru", "gru_back", "gru", "dense"], 547717),
])
def test_keras_json_architectures(arch, kinds, n_params, tmp_path):
    from poreover_amd.network import checkpoint as C
    cfg = C.ARCHITECTURES[arch]()
    p = tmp_path / (arch + ".json")
    p.write_text(json.dumps(cfg))
    spec = C.parse_model_json(str(p))
    assert [k for k, _ in spec] == kinds
    net = C.load_network(C.synthetic_weights(str(p), seed=0), str(p))
    assert net.kinds == kinds and net.n_params() == n_params
    assert net.flat_weights().size == n_params and net.flat_weights().dtype == np.float32
    # an InputLayer entry (newer Keras writes one) is not a layer with weights
    cfg2 = json.loads(json.dumps(cfg))
    cfg2["config"]["layers"].insert(0, {"class_name": "InputLayer", "config": {"batch_input_shape": [None, 1000, 1]}})
    assert [k for k, _ in C.parse_model_json(cfg2)] == kinds


def _mutate(arch, path, value):
    from poreover_amd.network import checkpoint as C
    cfg = C.ARCHITECTURES[arch]()
    node = cfg
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value
    return cfg


@pytest.mark.parametrize("arch,path,value,msg", [
    ("conv1_bigru3", ["config", "layers", 1, "config", "layer", "config", "units"], 64, "units"),
    ("conv1_gru5", ["config", "layers", 2, "config", "units"], 256, "units"),
    ("conv1_bigru3", ["config", "layers", 1, "config", "layer", "config", "reset_after"], False, "reset_after"),
    ("conv1_gru5", ["config", "layers", 1, "config", "reset_after"], False, "reset_after"),
    ("conv1_bigru3", ["config", "layers", 0, "config", "strides"], [2], "strides"),
    ("conv1_bigru3", ["config", "layers", 1, "config", "layer", "class_name"], "LSTM", "LSTM"),
    ("conv1_bigru3", ["config", "layers", 2, "class_name"], "LSTM", "LSTM"),
    ("conv1_bigru3", ["config", "layers", 4, "config", "units"], 6, "Dense"),
    ("conv1_bigru3", ["config", "layers", 1, "config", "layer", "config", "recurrent_activation"], "hard_sigmoid", "activation"),
])
def test_unsupported_models_refused(arch, path, value, msg):
    from poreover_amd.network import checkpoint as C
    with pytest.raises(C.NetworkError, match=msg):
        C.parse_model_json(_mutate(arch, path, value))


def test_weights_shape_mismatch_refused():
    from poreover_amd.network import checkpoint as C
    w = C.synthetic_weights(C.ARCHITECTURES["conv1_bigru3"](), seed=0)
    with pytest.raises(C.NetworkError):
        C.load_network(w, C.ARCHITECTURES["conv2_bigru3"]())
    with pytest.raises(C.NetworkError, match="no tensor"):
        C.load_network({}, None)


def test_call_requires_weights(tmp_path):
    from poreover_amd.__main__ import main
    with pytest.raises(SystemExit, match="--weights"):
        main(["call", FAST5_DIR, "--dir", str(tmp_path)])
    assert not list(tmp_path.iterdir())


def test_convert_npz_roundtrip(tmp_path):
    """an .npz of the checkpoint's tensor names (what convert writes) reads back exactly"""
    from poreover_amd.network import checkpoint as C
    w = C.synthetic_weights(None, seed=3)
    p = str(tmp_path / "w.npz")
    np.savez(p, **w)
    back = C.read_weights(p)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)


def test_oracle_keras_semantics_small():
    """the restatement itself: a 1-unit GRU by hand, and go_backwards order"""
    import _call_oracle as O
    x = np.array([[[1.0], [2.0], [-1.0]]])
    W = np.array([[0.5, -0.3, 0.8]])
    U = np.array([[0.2, 0.1, -0.4]])
    b = np.array([[0.1, 0.0, -0.2], [0.0, 0.3, 0.05]])
    h, out = 0.0, []
    for t in range(3):
        xz, xr, xh = x[0, t, 0] * W[0] + b[0]
        uz, ur, uh = h * U[0] + b[1]
        z = 1 / (1 + np.exp(-(xz + uz)))
        r = 1 / (1 + np.exp(-(xr + ur)))
        hh = np.tanh(xh + r * uh)
        h = z * h + (1 - z) * hh
        out.append(h)
    np.testing.assert_allclose(O.gru(x, W, U, b)[0, :, 0], out, rtol=1e-15)
    back = O.gru(x, W, U, b, go_backwards=True)[0, :, 0]
    fwd_of_reversed = O.gru(x[:, ::-1], W, U, b)[0, :, 0]
    np.testing.assert_array_equal(back, fwd_of_reversed)


@pytest.mark.skipif(not os.path.exists(REF_CKPT + ".index"), reason="reference checkout with its checkpoint not present")
def test_real_checkpoint_pair_identity(oracle):
    """the shipped weights (crc-checked) through the float64 restatement: read_316 and read_318 are the two strands of
    one molecule — their basecalls agree when one is reverse-complemented, not otherwise"""
    import _call_oracle as O
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import parse_fast5
    net = C.load_network(REF_CKPT)
    assert net.kinds == ["conv", "bigru", "bigru", "bigru", "dense"] and net.n_params() == 893189
    seqs = []
    for tag in ("read_316", "read_318"):
        _, p = O.basecall(net, parse_fast5(_fast5(tag))[1], 1000)
        seqs.append(O.greedy(p))
    rc = seqs[1][::-1].translate(str.maketrans("ACGT", "TGCA"))

    def ident(a, b):
        a1, a2 = oracle.global_pair_banded(a, b)
        return sum(x == y for x, y in zip(a1, a2)) / len(a1)

    assert ident(seqs[0], rc) >= 0.70
    assert ident(seqs[0], seqs[1]) <= 0.60
