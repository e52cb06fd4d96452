"""GPU: the guided, banded CTC forced aligner (po_label.hip) against tests/_label_oracle.py — map, status and score
compared with == on float64, no tolerance: every cell is one addition and one comparison, and a tolerance would hide
a wrong tie or a wrong row order — and make_labeled_data end to end."""
import os

import numpy as np
import pytest

import _label_oracle as LO
from poreover_amd import synth

pytestmark = pytest.mark.gpu

CODES = "ACGT"


@pytest.fixture(scope="module")
def batch():
    from poreover_amd import _lib, batch
    _lib.load()
    return batch


def _table(rng, T, sigma=1.5):
    return synth.log_softmax(rng.normal(0, sigma, (T, 5)))


def _seq(rng, L):
    return "".join(CODES[i] for i in rng.integers(4, size=L))


def _wiggly_guide(rng, T, L, amp):
    g = LO.default_guide(T, L) + rng.integers(-amp, amp + 1, size=T)
    return np.maximum.accumulate(np.clip(g, 0, L))


def _check(batch, ys, labs, guides, band, what=""):
    """device == oracle for every read of the batch; returns the device's answer"""
    maps, scores, status = batch.label_align_batch(ys, labs, guides, band_size=band)
    for i, (y, s) in enumerate(zip(ys, labs)):
        wm, wsc, wst = LO.label_align(y, s, None if guides is None else guides[i], band)
        tag = (what, i, len(y), len(s), band)
        assert status[i] == wst, tag
        assert scores[i] == wsc, tag + (float(scores[i]).hex(), float(wsc).hex())
        assert np.array_equal(maps[i], wm), tag
    return maps, scores, status


def _edge_batch(rng):
    """L = 0, L = 1, L = T, L > T, T = 1, T = 0, and ordinary reads"""
    ys, labs = [], []
    for T, L in [(1, 0), (1, 1), (1, 2), (0, 0), (0, 1), (7, 0), (7, 1), (7, 7), (7, 8), (64, 64), (65, 9), (128, 128),
                 (129, 40), (300, 300), (300, 2), (700, 90), (1000, 333), (63, 21), (2000, 200)]:
        ys.append(_table(rng, T))
        labs.append(_seq(rng, L))
    return ys, labs


@pytest.mark.parametrize("band", [1, 8, 32, 64, 200, 0])
def test_seeded_shapes(batch, band):
    rng = np.random.default_rng(100 + band)
    ys, labs = _edge_batch(rng)
    _check(batch, ys, labs, None, band, "diagonal")
    # a guide: wiggling around the diagonal (bands clipped at both ends), and exactly the oracle's optimum + noise
    guides = [_wiggly_guide(rng, len(y), len(s), 3) for y, s in zip(ys, labs)]
    _, _, st = _check(batch, ys, labs, guides, band, "guide")
    assert np.any(st == 0)
    # n = 1
    _check(batch, ys[-1:], labs[-1:], guides[-1:], band, "single")


def test_lengths_1_to_20000_in_one_batch(batch):
    """n = 257, lengths from 1 to 20 000 frames in one batch, with and without a guide, B = 32"""
    rng = np.random.default_rng(7)
    lens = np.unique(np.concatenate([[1, 2, 3, 63, 64, 65, 127, 128, 129, 20000], rng.integers(1, 3000, size=300)]))[:256]
    lens = np.concatenate([lens, [20000]])
    rng.shuffle(lens)
    assert len(lens) == 257 and lens.min() == 1 and lens.max() == 20000
    ys = [_table(rng, int(T)) for T in lens]
    labs = [_seq(rng, int(rng.integers(0, max(1, T // 3) + 1))) for T in lens]
    _check(batch, ys, labs, None, 32, "n257 diagonal")
    guides = [_wiggly_guide(rng, len(y), len(s), 5) for y, s in zip(ys, labs)]
    _check(batch, ys, labs, guides, 32, "n257 guide")
    _check(batch, ys[:40], labs[:40], guides[:40], 200, "n40 wide band")


def test_status_is_per_read(batch):
    """a guide jump the band cannot follow, a bad label character, a decreasing guide and a guide outside [0, L]: that
    read's status only; its neighbours are what they are alone"""
    from poreover_amd import _lib
    rng = np.random.default_rng(11)
    T, L = 600, 80
    ys = [_table(rng, T) for _ in range(6)]
    labs = [_seq(rng, L) for _ in range(6)]
    guides = [_wiggly_guide(rng, T, L, 2) for _ in range(6)]
    guides[1] = np.concatenate([np.zeros(300, np.int64), np.full(300, L, np.int64)])     # a jump of 80 > B
    labs[2] = labs[2][:40] + "N" + labs[2][41:]
    guides[3] = guides[3].copy(); guides[3][400] = guides[3][399] - 1
    guides[4] = guides[4].copy(); guides[4][-1] = L + 1
    for band in (8, 32, 100):
        _, _, st = _check(batch, ys, labs, guides, band, "status")
        # a jump of J states leaves no cell with an admitted predecessor exactly when J > 2 B + 1
        jump = _lib.E_ENVELOPE if L > 2 * band + 1 else 0
        assert list(st) == [0, jump, _lib.E_ARG, _lib.E_ARG, _lib.E_ARG, 0]
    # L > T without a band
    _, _, st = _check(batch, [ys[0][:50]], [labs[0]], None, 0, "L > T")
    assert st[0] == _lib.E_ENVELOPE


def _lagging_guide(T, L, hold, lag=0):
    """0 for `hold` frames, then a straight line to L - lag at the last frame"""
    t = np.arange(T)
    ramp = ((t - hold + 1) * (L - lag)) // max(T - hold, 1)
    return np.clip(np.where(t < hold, 0, ramp), 0, L).astype(np.int64)


@pytest.mark.parametrize("band,T,L", [(64, 600, 190),     # the whole state axis takes no more slots than the band's ring
                                      (200, 1500, 430),    # the same, B = 200
                                      (64, 4000, 1000),    # the band's own ring
                                      (200, 6000, 2000)])
def test_wide_band_binds(batch, band, T, L):
    """B >= 64 (the general kernel) with guides the band has to follow: a jump > 2 B + 1 loses every path, and a guide
    that lags or wiggles by about B gives an optimum that is not the unbanded one"""
    from poreover_amd import _lib
    rng = np.random.default_rng(band + T)
    ys = [_table(rng, T) for _ in range(5)]
    labs = [_seq(rng, L) for _ in range(5)]
    jump = 2 * band + 10
    assert jump < L
    g_jump = np.concatenate([np.zeros(T // 2, np.int64), np.full(T - T // 2, jump, np.int64)])
    g_jump[-1] = L
    guides = [g_jump,
              _lagging_guide(T, L, (2 * T) // 3),                       # every base in the last third
              np.clip(LO.default_guide(T, L) - (band - 3), 0, L),      # the diagonal sits at the band's upper edge
              np.minimum(LO.default_guide(T, L) + (band - 3), L),      # ... and at its lower edge
              _wiggly_guide(rng, T, L, band - 2)]
    _, scores, st = _check(batch, ys, labs, guides, band, "wide band")
    assert st[0] == _lib.E_ENVELOPE and not np.any(st[1:])
    free = batch.label_align_batch(ys, labs, None, band_size=0)
    assert not np.any(free[2])
    bound = [i for i in range(1, 5) if scores[i] != free[1][i]]
    print("B = %d, T = %d, L = %d: the band binds on guides %s" % (band, T, L, bound))
    # (with L < 3 B the shifted guides are clipped at 0 / L over most of the read and leave the optimum room)
    assert 1 in bound and (len(bound) >= 2 or L < 3 * band)


@pytest.mark.parametrize("band", [8, 32, 64, 0])
def test_exact_ties(batch, band):
    """y = log(1/5) everywhere: every comparison of a reachable cell is an exact tie, and a tie stays"""
    ys, labs, guides = [], [], []
    for T, L in [(12, 3), (200, 50), (640, 64), (1000, 1)]:
        ys.append(np.full((T, 5), np.log(0.2)))
        labs.append("ACGT" * (L // 4) + "ACGT"[:L % 4])
        guides.append(LO.default_guide(T, L))
    maps, _, st = _check(batch, ys, labs, None, band, "ties")
    _check(batch, ys, labs, guides, band, "ties guide")
    assert list(st) == [0, 0, 0, 0]


class _Hip:
    """device buffers through the HIP runtime the engine itself is linked to (torch's own runtime, brought up after the
    engine has used the device, finds no GPU)"""

    def __init__(self):
        import ctypes as C
        try:
            h = C.CDLL("libamdhip64.so")
        except OSError:
            h = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        self.h, self.C, self.bufs = h, C, []

    def alloc(self, nbytes):
        p = self.C.c_void_p()
        assert self.h.hipMalloc(self.C.byref(p), max(int(nbytes), 256)) == 0
        self.bufs.append(p)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            assert self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p

    def get(self, p, shape, dtype):
        out = np.zeros(shape, dtype=dtype)
        if out.nbytes:
            assert self.h.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self):
        assert self.h.hipDeviceSynchronize() == 0
        for p in self.bufs:
            self.h.hipFree(p)
        self.bufs = []


def _device_call(lib, ys, labs, guides, band):
    """po_label_align_batch on device pointers with a workspace of exactly the queried size"""
    from poreover_amd import batch as B
    y, off, Cc = B.pack_rows(ys, 5)
    lb, lo = B._pack_labels(labs)
    n = len(ys)
    hip = _Hip()
    try:
        d_y, d_off, d_lo, d_lb = hip.put(y), hip.put(off), hip.put(lo), hip.put(lb)
        d_g = None
        if guides is not None:
            d_g = hip.put(np.concatenate([np.asarray(x, np.int32) for x in guides] + [np.zeros(1, np.int32)]))
        nl = max(int(lo[-1]), 1)
        d_map, d_sc, d_st = hip.alloc(4 * nl), hip.alloc(8 * n), hip.alloc(4 * n)
        mx = int(np.diff(off).max())
        wsb = int(lib.po_label_align_workspace_bytes(n, int(off[-1]), mx, int(lo[-1]), band))
        d_ws = hip.alloc(wsb)
        rc = lib.po_label_align_batch(d_y, d_off, n, Cc, b"ACGT", band, d_lb, d_lo, d_g, d_map, d_sc, d_st, d_ws, wsb, None)
        assert rc == 0, rc
        assert hip.h.hipDeviceSynchronize() == 0
        mp = hip.get(d_map, nl, np.int32)
        sc, st = hip.get(d_sc, n, np.float64), hip.get(d_st, n, np.int32)
    finally:
        hip.free()
    return [mp[lo[i]:lo[i + 1]].astype(np.int64) for i in range(n)], sc, st, wsb


def test_batch_position_and_entry_point(batch):
    """a read alone == the same read among 256 others, at two positions; device-pointer entry == host-pointer entry"""
    from poreover_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(21)
    ys = [_table(rng, int(T)) for T in rng.integers(1, 1500, size=256)]
    labs = [_seq(rng, int(rng.integers(0, len(y) // 4 + 1))) for y in ys]
    guides = [_wiggly_guide(rng, len(y), len(s), 4) for y, s in zip(ys, labs)]
    y0 = synth.synth_render(rng.integers(4, size=330), 3000, seed=5)[0]
    s0 = _seq(rng, 330)
    g0 = _wiggly_guide(rng, 3000, 330, 6)
    for band in (32, 8, 100):
        alone = batch.label_align_batch([y0], [s0], [g0], band_size=band)
        for pos in (0, 100, 256):
            got = batch.label_align_batch(ys[:pos] + [y0] + ys[pos:], labs[:pos] + [s0] + labs[pos:],
                                          guides[:pos] + [g0] + guides[pos:], band_size=band)
            assert np.array_equal(got[0][pos], alone[0][0]) and got[1][pos] == alone[1][0] and got[2][pos] == alone[2][0]
        host = batch.label_align_batch(ys + [y0], labs + [s0], guides + [g0], band_size=band)
        dm, dsc, dst, _ = _device_call(lib, ys + [y0], labs + [s0], guides + [g0], band)
        assert np.array_equal(dst, host[2])
        assert np.array_equal(dsc.view(np.uint64), host[1].view(np.uint64))
        assert all(np.array_equal(a, b) for a, b in zip(dm, host[0]))
    # no guide through the device-pointer entry
    host = batch.label_align_batch(ys[:50], labs[:50], None, band_size=32)
    dm, dsc, dst, _ = _device_call(lib, ys[:50], labs[:50], None, 32)
    assert np.array_equal(dst, host[2]) and np.array_equal(dsc.view(np.uint64), host[1].view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(dm, host[0]))


def _cap(n, total_rows, total_labels, B):
    return total_rows * (2 * (-(-(2 * B + 1) // 64)) * 8 + 16) + 32 * total_labels + 64 * n + 2 ** 20


def test_workspace_cap():
    from poreover_amd import _lib
    lib = _lib.load()
    for n, rows, mx, labels in [(1, 200000, 200000, 21000), (8, 1600000, 200000, 168000), (257, 700000, 20000, 90000),
                                (10000, 3000000, 600, 400000), (1, 1, 1, 0)]:
        for B in (1, 8, 31, 32, 63, 64, 200, 5000):
            got = lib.po_label_align_workspace_bytes(n, rows, mx, labels, B)
            assert 0 < got <= _cap(n, rows, labels, B), (n, rows, labels, B, got)
    assert lib.po_label_align_workspace_bytes(1, 200000, 200000, 21000, 32) < 10 * 2 ** 20


def test_whole_reads(batch):
    """8 reads of T = 200 000, L about 21 000, B = 32, the guide from the Viterbi basecall"""
    from poreover_amd import _lib
    from poreover_amd.network import make_labeled_data as mld
    lib = _lib.load()
    T = 200000
    ys, labs, guides = [], [], []
    for k in range(8):
        rng = np.random.default_rng(4000 + k)
        parent = rng.integers(4, size=21000)
        read = synth._mutate(rng, parent)
        y, _ = synth.synth_render(read, T, seed=4100 + k)
        ys.append(y)
        labs.append("".join(CODES[c] for c in parent))
    called, fmaps, vst = batch.viterbi_batch(ys, return_map=True)
    assert not np.any(vst)
    cols = batch.align_batch([(c, s) for c, s in zip(called, labs)])
    for (a1, a2), fm in zip(cols, fmaps):
        consumed, ident = mld.consumed_from_columns(a1, a2)
        assert ident > 0.85
        guides.append(mld.guide_from_alignment(fm, consumed, T))
    dm, dsc, dst, wsb = _device_call(lib, ys, labs, guides, 32)
    assert wsb <= _cap(8, 8 * T, sum(len(s) for s in labs), 32)
    print("workspace for 8 x 200 000 frames: %.1f MB" % (wsb / 1e6))
    assert not np.any(dst)
    for i in range(8):
        wm, wsc, wst = LO.label_align(ys[i], labs[i], guides[i], 32)
        assert wst == 0 and dsc[i] == wsc and np.array_equal(dm[i], wm), i


# ---------------------------------------------------------------------------------------------- make_labeled_data


def _planted_reads(n, seed, mean_len=3000):
    """a synth_genome, reads cut from it on both strands, each rendered to a posterior table (about 9.4 frames per base)
    with a random signal of the same length"""
    names, seqs, _ = synth.synth_genome(seed, contig_lengths=(120000, 80000), n_runs=2, run_len=(20, 60), repeat_len=0)
    reads = synth.synth_mapping_reads(seqs, n, seed=seed + 1, mean_len=mean_len, sigma=0.3, err=(0.03, 0.12), random_frac=0.1,
                                      min_len=400, max_len=6000)
    rng = np.random.default_rng(seed + 2)
    tables, signals = [], []
    for k, r in enumerate(reads):
        s = r["seq"].replace("N", "A")
        T = int(len(s) * 9.4)
        tables.append(synth.synth_render(s, T, seed=seed + 10 + k)[0])
        signals.append(rng.standard_normal(T))
    return names, seqs, reads, tables, signals


def _oracle_pipeline(batch, aligner, signals, tables, window, band, min_identity):
    """label_reads restated with the oracle's aligner, guide and window rule, on the same Viterbi calls and hits"""
    called, fmaps, _ = batch.viterbi_batch(tables, return_map=True)
    hits = aligner.map_batch(called)
    rows, labels, lens, per_read = [], [], [], []
    stats = {"unmapped": 0, "low_identity": 0, "band_lost": 0}
    comp = str.maketrans("ACGT", "TGCA")
    for i, h in enumerate(hits):
        if h is None:
            stats["unmapped"] += 1
            per_read.append(None)
            continue
        if h.mlen / h.blen < min_identity:
            stats["low_identity"] += 1
            per_read.append(None)
            continue
        truth = aligner.seq(h.ctg, h.r_st, h.r_en)
        cigar = [tuple(c) for c in h.cigar]
        if h.strand < 0:
            truth, cigar = truth.translate(comp)[::-1], cigar[::-1]
        consumed = LO.consumed_from_cigar(cigar, h.q_en - h.q_st)
        fr = fmaps[i][h.q_st:h.q_en]
        f0, f1 = int(fr[0]), int(fr[-1])
        guide = LO.guide_from_alignment(fr - f0, consumed, f1 - f0 + 1)
        mp, _, st = LO.label_align(tables[i][f0:f1 + 1], "".join(c if c in CODES else "A" for c in truth), guide, band)
        if st != 0:
            stats["band_lost"] += 1
            per_read.append(None)
            continue
        r, l, n = LO.windows(signals[i], mp + f0, truth, f0, f1, window)
        rows += r; labels += l; lens += n
        per_read.append((truth, l, n))
    return (np.stack(rows), np.array(labels, np.int32), np.array(lens, np.int32), stats, per_read)


def test_label_reads_end_to_end(batch, tmp_path):
    from poreover_amd import mapping
    from poreover_amd.network import make_labeled_data as mld
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import train
    names, seqs, reads, tables, signals = _planted_reads(24, 77)
    assert any(r["random"] for r in reads) and any(r["strand"] < 0 for r in reads) and any(r["strand"] > 0 for r in reads)
    aligner = mapping.Aligner.from_sequences(names, seqs)
    window = 100
    try:
        sig, lab, lens, stats = mld.label_reads(signals, tables, aligner=aligner, window=window, band_size=32, min_identity=0.8)
        w_sig, w_lab, w_lens, w_stats, per_read = _oracle_pipeline(batch, aligner, signals, tables, window, 32, 0.8)
        # a high identity bar: every read is counted as too poor, none contributes
        none = mld.label_reads(signals, tables, aligner=aligner, window=window, band_size=32, min_identity=0.9999)
    finally:
        aligner.close()
    print(mld.summary_line(stats))
    assert np.array_equal(sig, w_sig) and sig.dtype == np.float32
    assert np.array_equal(lab, w_lab) and np.array_equal(lens, w_lens)
    assert {k: stats[k] for k in w_stats} == w_stats and stats["reads"] == len(reads) and stats["windows"] == len(sig)
    assert stats["unmapped"] >= sum(r["random"] for r in reads)
    for i, r in enumerate(reads):
        if r["random"]:
            assert per_read[i] is None
    assert none[3]["windows"] == 0 and len(none[0]) == 0 and none[3]["low_identity"] + none[3]["unmapped"] == len(reads)
    assert len(sig) > 100
    assert np.all(lens >= 1) and np.all(lens <= window)
    # the labels of a read's consecutive windows, concatenated, are a contiguous slice of its truth segment
    for pr in per_read:
        if pr is None or not pr[1]:
            continue
        truth, l, n = pr
        if "N" in truth:
            continue   # a window with an N is dropped: the read's labels are then slices either side of it
        assert "".join(CODES[c] for c in l) in truth
    # write, reload, train three steps
    path = mld.write_npz(str(tmp_path / "labeled"), sig, lab, lens)
    s2, l2, n2 = train.load_data(path)
    assert np.array_equal(s2, sig) and np.array_equal(l2, lab) and np.array_equal(n2, lens)
    train.check_labels(l2, n2, s2.shape[1], False)
    cfg = C.architecture("conv1_bigru3", filters=32)
    net = C.load_network(train.init_weights(cfg, 3), cfg)
    off = np.concatenate([[0], np.cumsum(n2)])
    with train.Trainer(net, 16, window) as tr:
        for step in range(3):
            idx = np.arange(16 * step, 16 * step + 16)
            loss = tr.step(s2[idx], [l2[off[i]:off[i + 1]] for i in idx])
            assert loss.shape == (16,) and np.all(np.isfinite(loss))


FAST5_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast5")


def test_cli_on_fast5(batch, tmp_path, capsys):
    import glob
    from poreover_amd.decoding import decode
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network import make_labeled_data as mld
    from poreover_amd.network import network, train
    files = sorted(glob.glob(os.path.join(FAST5_DIR, "*.fast5")))
    assert len(files) == 3
    probs_dir = tmp_path / "probs"
    probs_dir.mkdir()
    signals, tables, truths = [], [], []
    with open(tmp_path / "truth.fasta", "w") as fa:
        for k, f in enumerate(files):
            sig = np.asarray(network.parse_fast5(f)[1], dtype=np.float64)
            rng = np.random.default_rng(300 + k)
            seq = "".join(CODES[c] for c in rng.integers(4, size=len(sig) // 10))
            y, _ = synth.synth_render(seq, len(sig), seed=310 + k)
            stem = os.path.splitext(os.path.basename(f))[0]
            np.save(probs_dir / (stem + ".npy"), np.exp(y))
            fa.write(">%s some description\n" % stem)
            for a in range(0, len(seq), 60):
                fa.write(seq[a:a + 60] + "\n")
            signals.append(sig)
            tables.append(np.asarray(decode.load_logits(str(probs_dir / (stem + ".npy")), flatten=True), dtype=np.float64))
            truths.append(seq)
    out = str(tmp_path / "cli")
    stats = mld.main(["--input", FAST5_DIR, "--probs", str(probs_dir), "--truth", str(tmp_path / "truth.fasta"),
                      "--output", out, "--unroll", "200", "--threads", "4"])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and line[0].startswith("make_labeled_data: reads in 3 / unmapped 0 / low identity 0 / band lost 0")
    want = mld.label_reads(signals, tables, truths=truths, window=200)
    s, l, n = train.load_data(out + ".npz")
    assert np.array_equal(s, want[0]) and np.array_equal(l, want[1]) and np.array_equal(n, want[2])
    assert stats["windows"] == len(s) > 0 and s.shape[1] == 200
    # the `call` route: synthetic weights call garbage, so only the plumbing is checked
    cfg = C.architecture("conv1_bigru3", filters=32)
    wpath = str(tmp_path / "weights.npz")
    C.write_weights(wpath, C.load_network(C.synthetic_weights(cfg), cfg))
    mpath = str(tmp_path / "model.json")
    import json
    with open(mpath, "w") as f:
        json.dump(cfg, f)
    out2 = str(tmp_path / "cli2")
    stats2 = mld.main(["--input", FAST5_DIR, "--weights", wpath, "--model", mpath, "--truth", str(tmp_path / "truth.fasta"),
                       "--output", out2, "--min_identity", "0"])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and line[0].startswith("make_labeled_data: reads in 3 / ")
    with np.load(out2 + ".npz") as z:
        assert z["signal"].dtype == np.float32 and z["signal"].ndim == 2 and z["signal"].shape[1] == 100
        assert z["labels"].dtype == np.int32 and z["row_lengths"].dtype == np.int32
        assert int(z["row_lengths"].sum()) == len(z["labels"]) and len(z["row_lengths"]) == len(z["signal"]) == stats2["windows"]
