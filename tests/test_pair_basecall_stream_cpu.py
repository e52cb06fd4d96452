"""`pair-basecall` over several devices without a GPU: the group planner — po_pair_basecall_group_plan
through the library, which loads without a device, against its Python twin pair_basecall.engine_group_plan —, the command's
refusals that come before any file is read, the chunked driver of `pair-basecall --gpus` against a stand-in engine, and the
new entries' declarations."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("po_pair_basecaller_create", "po_pair_basecaller_destroy", "po_pair_basecaller_run_f32", "po_pair_basecaller_run_raw",
       "po_pair_basecaller_stats", "po_pair_basecall_group_plan")

# Case A's read lengths (tests/_pair_basecall_cases.py) and one read far larger than the rest
LENS = [333, 333, 104, 104, 73, 41, 333, 60000]
PAIRS = [(0, 1), (1, 0), (2, 3), (0, 0), (4, 5), (7, 7), (0, 6), (3, 2), (1, 0), (5, 4)]


def _options(kind="poreover", beam_width=5):
    from poreover_amd import _marshal
    return _marshal.pair_options(kind, beam_width, "row_col", 5, "banded", False, 50)


def _lib_plan(lens, pairs, opt, fastq, band, budget, ndev):
    from poreover_amd import _lib
    lib = _lib.load(require_gpu=False)
    a = np.ascontiguousarray(lens, dtype=np.int64)
    idx = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1)) if pairs else np.zeros(2, dtype=np.int32)
    cap = max(len(pairs), 1)
    first, count = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    g = lib.po_pair_basecall_group_plan(a.ctypes.data, len(a), idx.ctypes.data, len(pairs), C.byref(opt), 1 if fastq else 0, band,
                                        int(budget), ndev, first.ctypes.data, count.ctypes.data, len(pairs))
    assert g >= 0, lib.po_last_error()
    return [(int(first[i]), int(count[i])) for i in range(g)]


def _py_plan(lens, pairs, opt, fastq, band, budget, ndev):
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall as PB
    lib = _lib.load(require_gpu=False)
    ws = lambda n, t1, t2, m1, m2: int(lib.po_pair_decode_workspace_bytes(n, t1, t2, m1, m2, 5, C.byref(opt)))
    return PB.engine_group_plan(pairs, lens, ws, budget=budget, ndev=ndev,
                                qual_bytes=PB.qual_bytes_query(lib, band, opt.model) if fastq else None)


def _need(lens, pairs, opt, fastq, band):
    """the resident bytes of `pairs` as one group"""
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall as PB
    lib = _lib.load(require_gpu=False)
    t = [sum(lens[a] for a, _ in pairs), sum(lens[b] for _, b in pairs)]
    m = [max(lens[a] for a, _ in pairs), max(lens[b] for _, b in pairs)]
    need = sum(lens[r] for r in {r for p in pairs for r in p}) * 24 + sum(t) * 40
    need += int(lib.po_pair_decode_workspace_bytes(len(pairs), t[0], t[1], m[0], m[1], 5, C.byref(opt)))
    if fastq:
        need += PB.qual_bytes_query(lib, band, opt.model)(len(pairs), t[0], t[1], m[0], m[1])
    return need


def _covers(groups, n):
    at = 0
    for f, c in groups:
        assert f == at and c >= 1
        at += c
    assert at == n


@pytest.mark.parametrize("fastq,band", [(False, 0), (True, 10), (True, 0)])
@pytest.mark.parametrize("ndev", (1, 2, 8))
def test_planner_equals_its_python_twin(ndev, fastq, band):
    opt = _options()
    small = PAIRS[:5]                                                  # without the large read
    one = _need(LENS, small, opt, fastq, band)
    two = _need(LENS, small[:2], opt, fastq, band)
    for pairs in (small, PAIRS):
        for budget in (1, two - 1, two, (one + two) // 2, one - 1, one, 10 ** 13):
            got = _lib_plan(LENS, pairs, opt, fastq, band, budget, ndev)
            assert got == _py_plan(LENS, pairs, opt, fastq, band, budget, ndev), (budget, got)
            _covers(got, len(pairs))
            if budget == 1:
                assert got == [(k, 1) for k in range(len(pairs))]      # every pair alone
    # the budget of Case A's first two pairs: they share reads 0 and 1 with the group after them ((0, 0) is the fourth pair)
    got = _lib_plan(LENS, small, opt, fastq, band, two, 1)
    assert got[0] == (0, 2) and len(got) >= 2
    # a pair too large for the budget goes alone, its neighbours are grouped as before
    got = _lib_plan(LENS, PAIRS, opt, fastq, band, one, 1)
    assert (5, 1) in got and got[0][1] > 1
    assert _lib_plan(LENS, [], opt, fastq, band, one, ndev) == _py_plan(LENS, [], opt, fastq, band, one, ndev) == []


def test_the_frame_cap_is_for_several_devices_alone():
    """ndev == 1: the budget alone bounds a group (a second group there is a second full recurrence);
    ndev > 1: at most ceil(pair-side frames / (2 ndev)) pair-side frames per group, one pair at least"""
    opt = _options()
    pairs = PAIRS[:5]
    frames = [LENS[a] + LENS[b] for a, b in pairs]
    assert _lib_plan(LENS, pairs, opt, False, 0, 10 ** 13, 1) == [(0, len(pairs))]
    for ndev in (2, 8):
        share = -(-sum(frames) // (2 * ndev))
        got = _lib_plan(LENS, pairs, opt, False, 0, 10 ** 13, ndev)
        assert got == _py_plan(LENS, pairs, opt, False, 0, 10 ** 13, ndev) and len(got) >= 2
        for f, c in got:
            assert c == 1 or sum(frames[f:f + c]) <= share
            if f + c < len(pairs):
                assert sum(frames[f:f + c + 1]) > share                # greedy: the next pair would not have fitted
    assert _lib_plan(LENS, pairs, opt, False, 0, 10 ** 13, 8) == [(k, 1) for k in range(len(pairs))]


def test_planner_refusals():
    from poreover_amd import _lib
    lib = _lib.load(require_gpu=False)
    opt = _options()
    a = np.array([5, 5], dtype=np.int64)
    idx = np.array([0, 2], dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)
    call = lambda ndev, budget: lib.po_pair_basecall_group_plan(a.ctypes.data, 2, idx.ctypes.data, 1, C.byref(opt), 0, 0, budget, ndev,
                                                                out.ctypes.data, out.ctypes.data, 1)
    assert call(1, 0) == _lib.E_ARG and b"pair 0 names read 2 (reads 0 to 1)" in lib.po_last_error()
    idx[1] = 1
    assert call(0, 0) == _lib.E_ARG and b"ndev 0" in lib.po_last_error()
    assert call(1, -1) == _lib.E_ARG and b"resident_bytes -1" in lib.po_last_error()
    assert call(1, 0) == 1                                              # resident_bytes 0: the default budget


def test_group_rule_under_sanitizers(tmp_path):
    """csrc/po_pair_basecall_group_rules.h alone (no HIP) against a brute-force restatement, under ASan and UBSan"""
    import subprocess
    exe = str(tmp_path / "pair_group_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "pair_group_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def _parse(argv):
    from poreover_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_parser():
    a = _parse(["pair-basecall", "pairs.txt", "--weights", "w.npz"])
    assert a.gpus is None and a.readers == 4 and a.chunk_pairs == 256
    a = _parse(["pair-basecall", "pairs.txt", "--weights", "w.npz", "--gpus", "0", "--readers", "16", "--chunk_pairs", "1"])
    assert (a.gpus, a.readers, a.chunk_pairs) == (0, 16, 1)


@pytest.mark.parametrize("readers", (0, 17))
def test_readers_outside_1_to_16_is_refused(readers, tmp_path):
    """before --weights (no such file) and the pairs file (no such file) are opened"""
    from poreover_amd.network import pair_basecall as PB
    a = _parse(["pair-basecall", str(tmp_path / "none.txt"), "--weights", str(tmp_path / "none.npz"), "--gpus", "1",
                "--readers", str(readers)])
    with pytest.raises(SystemExit, match=r"pair-basecall: --readers %d must be 1 to 16" % readers):
        PB.pair_basecall(a)


def test_gpus_outside_the_visible_devices_is_refused(tmp_path, monkeypatch):
    from poreover_amd import _lib
    from poreover_amd.network import pair_basecall as PB
    argv = ["pair-basecall", str(tmp_path / "none.txt"), "--weights", str(tmp_path / "none.npz")]
    with pytest.raises(SystemExit, match="pair-basecall: --gpus must not be negative"):
        PB.pair_basecall(_parse(argv + ["--gpus", "-1"]))

    class Two:
        @staticmethod
        def po_device_count():
            return 2
    monkeypatch.setattr(_lib, "load", lambda require_gpu=True: Two)
    with pytest.raises(SystemExit, match="pair-basecall: --gpus 3, but 2 devices are visible"):
        PB.pair_basecall(_parse(argv + ["--gpus", "3"]))
    with pytest.raises(SystemExit, match="pair-basecall: --chunk_pairs 0 must be 1 at least"):
        PB.pair_basecall(_parse(argv + ["--gpus", "2", "--chunk_pairs", "0"]))
    # the refusals of check_args come first, as worded
    with pytest.raises(SystemExit, match="pair-basecall: --threads 2: one device per call"):
        PB.pair_basecall(_parse(argv + ["--gpus", "3", "--threads", "2"]))


# ---- the chunked driver on a stand-in engine: read k's raw signal is k + 1 samples of the value k; a pair's record names them
READS = ["r%d" % k for k in range(7)]
LINES = [("r0", "r1"), ("r1.npy", "r0.fast5"), ("r2", "r2"), ("r0", "r3"), ("r4", "r5"), ("r5", "r4"), ("r6", "r0")]


class Stand:
    def __init__(self):
        self.log, self.lock, self.engines = [], threading.Lock(), []

    def read(self, path):
        k = int(os.path.basename(path)[1:-len(".fast5")])
        with self.lock:
            self.log.append(("read", k))
        return b"id%d" % k, np.full(k + 1, k, dtype=np.int16), 0.0, 1.0, 1.0

    def engine(self, net, raws, pairs, channels, **kw):
        with self.lock:
            self.log.append(("run", tuple(int(r[0]) for r in raws)))
        self.engines.append(kw["engines"])
        assert kw["devices"] == [0, 1] and all(len(c) == 3 for c in channels)
        out = []
        for a, b in pairs:
            s1, s2 = "ACGT"[int(raws[a][0]) % 4] * len(raws[a]), "ACGT"[int(raws[b][0]) % 4] * len(raws[b])
            status = -3 if int(raws[a][0]) == 6 else 0                   # the pair naming r6 first: a per-pair refusal
            out.append({"status": status, "seq1": s1, "seq2": s2, "consensus": s1 + s2 if status == 0 else None,
                        "length1": len(s1), "length2": len(s2), "sequence_identity": 0.5, "skipped": 0 if status == 0 else 1})
        with self.lock:
            self.log.append(("done", tuple(int(r[0]) for r in raws)))
        return out


def _drive(tmp_path, monkeypatch, name, extra):
    from poreover_amd.network import pair_basecall as PB
    stand = Stand()
    monkeypatch.setattr(PB, "read_fast5_raw", stand.read)
    monkeypatch.setattr(PB, "pair_basecall_raw", stand.engine)
    args = _parse(["pair-basecall", "pairs.txt", "--dir", str(tmp_path), "--weights", "w.npz", "--out", str(tmp_path / name),
                   "--gpus", "2"] + extra)
    records = PB._pair_basecall_stream(args, None, [list(p) for p in LINES], [0, 1])
    return stand, records, [open(str(tmp_path / name) + ext).read() for ext in (".1d.fasta", ".2d.fasta", ".log")]


def test_chunked_driver(tmp_path, monkeypatch):
    stand, records, files = _drive(tmp_path, monkeypatch, "two", ["--chunk_pairs", "2", "--readers", "3"])
    runs = [e[1] for e in stand.log if e[0] == "run"]
    # chunks of two lines; a chunk's distinct files in first-seen order: r2 (named twice in its chunk) once, r0 in three chunks
    assert runs == [(0, 1), (2, 0, 3), (4, 5), (6, 0)]
    reads = [e[1] for e in stand.log if e[0] == "read"]
    assert sorted(reads) == sorted(k for run in runs for k in run) and reads.count(0) == 3 and reads.count(2) == 1
    # two chunks alive at most: chunk c + 2 is not read before chunk c is done
    for c in range(2, len(runs)):
        new = [k for k in runs[c] if k not in runs[c - 1] and k not in runs[c - 2]]
        assert new
        for k in new:
            assert stand.log.index(("read", k)) > stand.log.index(("done", runs[c - 2]))
    # one dict of engines serves every chunk
    assert all(e is stand.engines[0] for e in stand.engines) and len(stand.engines) == 4
    # input order across the chunks; the refused pair is logged like any other per-pair refusal and has no record
    assert len(records) == len(LINES)
    log = files[2].split("\n")
    assert log[0] == "# PoreOver pair-decode" and "'chunk_pairs'" not in log[1] and "'readers'" not in log[1] and "'gpus': 2" in log[1]
    assert [tuple(l.split("\t")[:2]) for l in log[3:-1]] == LINES
    assert log[3 + 6].split("\t")[2:] == ["7", "1", "", "1"]
    assert files[0].count(">") == 2 * 6 and files[0].startswith(">r0\nA\n>r1\nCC\n")
    assert [l for l in files[1].split("\n") if l.startswith(">")] == \
        [">consensus;%s;%s" % (a.split(".")[0], b.split(".")[0]) for a, b in LINES[:6]]
    # another chunking writes the same bytes
    _, _, other = _drive(tmp_path, monkeypatch, "one", ["--chunk_pairs", "1", "--readers", "1"])
    _, _, whole = _drive(tmp_path, monkeypatch, "all", [])
    for a, b, c in zip(files, other, whole):
        assert a.replace(str(tmp_path / "two"), "X") == b.replace(str(tmp_path / "one"), "X") == c.replace(str(tmp_path / "all"), "X")


def test_new_symbols_are_exported_and_prototyped():
    from poreover_amd import _lib
    lib = _lib.load(require_gpu=False)
    text = open(os.path.join(REPO, "include", "poreover_hip.h")).read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        at = text.index(" %s(" % name)
        decl = text[at:text.index(");", at)]
        assert decl.count(",") + 1 == len(_lib.PROTOTYPES[name][1]), name
    # the options struct, field by field as the header lists them
    at = text.index("typedef struct po_pair_basecaller_options {")
    body = text[at:text.index("} po_pair_basecaller_options;")].split("{", 1)[1]
    fields = [f.strip() for line in body.split(";") for f in line.strip().split(" ", 1)[-1].split(",") if line.strip()]
    assert fields == [f for f, _ in _lib.PairBasecallerOptions._fields_]
    assert C.sizeof(_lib.PairBasecallerOptions) == 4 * 4 + C.sizeof(_lib.PairOptions) + 5 * 4 + 8
    for name in ("PairBasecaller", "pair_basecall_raw", "engine_group_plan"):
        from poreover_amd.network import pair_basecall as PB
        assert name in PB.__all__ and hasattr(PB, name)
