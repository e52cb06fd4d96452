"""GPU: the kernels of po_map.hip at their edges, stage by stage, against the CPU restatement (tests/_map_oracle.py) bit
for bit and, where the band is the whole matrix, against a plain Gotoh matrix.  The cases come from
tests/_map_edge_cases.py; tests/test_map_edge_cases_cpu.py shows without a GPU that each reaches the edge it is named
after (the sort thresholds, the 64th predecessor, the band masks and shifts, the quantile's rank, ...)."""
import ctypes as C
import re

import numpy as np
import pytest

import _map_edge_cases as E
import _map_oracle as O
import _pairs_oracle as PO
from poreover_amd import mapping

pytestmark = pytest.mark.gpu

FIELDS = ("mapped", "ctg", "strand", "score", "r_st", "r_en", "q_st", "q_en", "mlen", "blen", "nm", "n_anchors", "n_chain",
          "chain_score")


def _aligner(names, seqs):
    from poreover_amd import _lib
    _lib.load()
    return mapping.Aligner.from_sequences(names, seqs)


def _records(recs, ops, n, ctg=None):
    """[(fields..., op bytes)] of n device records; ctg: the value to put in place of the record's own"""
    out = []
    for i in range(n):
        r = recs[i]
        f = [int(getattr(r, k)) for k in FIELDS]
        if ctg is not None:
            f[1] = ctg
        out.append((tuple(f), bytes(ops[r.op_off:r.op_off + r.n_ops]) if r.mapped else b""))
    return out


def _ops_of_cs(cs):
    """the op bytes that a short cs string spells (0 M, 1 X, 2 I, 3 D)"""
    out = []
    for m in re.finditer(r":(\d+)|\*[a-z]{2}|\+([a-z]+)|-([a-z]+)", cs):
        t = m.group(0)
        out += [0] * int(m.group(1)) if t[0] == ":" else [1] if t[0] == "*" else [2 if t[0] == "+" else 3] * (len(t) - 1)
    return bytes(out)


def _check_record(r, ops, read, ctg_seq):
    """what holds for every mapped record without an oracle"""
    o = ops[r.op_off:r.op_off + r.n_ops]
    assert r.n_ops > 0 and o[0] in (0, 1) and o[-1] in (0, 1)
    cnt = [int(v) for v in np.bincount(o, minlength=4)]
    assert cnt[0] + cnt[1] + cnt[2] == r.q_en - r.q_st and 0 <= r.q_st < r.q_en <= len(read)
    assert cnt[0] + cnt[1] + cnt[3] == r.r_en - r.r_st and 0 <= r.r_st < r.r_en <= len(ctg_seq)
    assert (r.mlen, r.blen, r.nm) == (cnt[0], sum(cnt), cnt[1] + cnt[2] + cnt[3])
    Q = O.reverse_complement_q(read) if r.strand < 0 else read
    qs = len(read) - r.q_en if r.strand < 0 else r.q_st
    assert O.rescore(list(o), O.codes(Q), O.codes(ctg_seq), qs, r.r_st) == r.score >= O.MIN_SCORE


def _anchors_of(dbg, lo, n):
    key = dbg["anchor_key"][lo:lo + n].astype(np.int64)
    if n == 0:
        return np.zeros((0, 4), np.int64)
    return np.stack([(key >> 32) >> 1, (key >> 32) & 1, key & 0xffffffff, dbg["anchor_y"][lo:lo + n].astype(np.int64)],
                    axis=1)


def _check_stages(names, reads, recs, dbg, want, hits=None):
    """anchors in order, chain, band starts and score of every read against the restatement's detail"""
    ao = co = 0
    off = dbg["offsets"]
    for i, (hit, info) in enumerate(want):
        r, a = recs[i], info["anchors"]
        assert r.n_anchors == len(a), names[i]
        assert np.array_equal(_anchors_of(dbg, ao, len(a)), a), names[i]
        ao += len(a)
        assert (r.n_chain, r.chain_score) == (len(info["chain"]), info["chain_score"]), names[i]
        assert list(dbg["chain"][co:co + r.n_chain]) == list(info["chain"]), names[i]
        co += r.n_chain
        if "band_lo" in info:
            assert np.array_equal(dbg["band_lo"][off[i]:off[i + 1]], info["band_lo"]), names[i]
            assert r.score == info["score"], names[i]
        assert bool(r.mapped) == (hit is not None), names[i]
        if hits is not None:
            assert hits[i] == hit, names[i]


# --------------------------------------------------------------------------------------------------------- 1. sketch

@pytest.mark.parametrize("total", E.SKETCH_TOTALS)
def test_sketch_at_sequence_edges_and_scan_tiles(total):
    """map_hash / map_minflag / the scan / map_emit: one call over sequences of every length around k and k + w - 1, empty
    ones first, last and twice in a row (seq_of shares their offsets), N at the ends and everywhere, tied hashes, runs
    shorter than w; the call's total length on both sides of the scan's tile.  A lower-case sequence has no k-mer: §12's
    k-mers exist on the bytes A, C, G, T alone, and upper-casing is the readers' work (decision 6)."""
    items = E.sketch_lists()[total]
    got = mapping.sketch_device([s for _, s in items])
    assert len(got) == len(items)
    for (name, s), (h, p, st) in zip(items, got):
        wh, wp, wst = O.sketch(s)
        assert np.array_equal(h.astype(np.int64), wh), name
        assert np.array_equal(p.astype(np.int64), wp), name
        assert np.array_equal(st.astype(np.int64), wst.astype(np.int64)), name
    assert len(dict(items)["lower_case"]) == 40 and len(got[[n for n, _ in items].index("lower_case")][0]) == 0


# --------------------------------------------------------------------------------------------------------- 2. anchors

def test_anchor_counts_on_the_sort_thresholds():
    """map_anchor_* and map_sort_kernel: exactly 1, 2, 1024, 2047, 2048 (the last sort in LDS), 2049 (the first in the
    global slice), 4096, 4097 and more than 5000 anchors, none at all, and a hash above max_occ, in one call"""
    names, seqs, _ = E.anchor_index()
    idx = E.oracle_index("anchor")
    al = _aligner(names, seqs)
    assert al.max_occ == idx.max_occ == 10
    cases = E.anchor_reads()
    reads = [s for _, s, _ in cases]
    recs, ops, dbg = al.map_raw(reads, debug=True)
    ao = co = n_mapped = 0
    for i, (name, s, a) in enumerate(cases):
        r = recs[i]
        assert r.n_anchors == len(a), name
        assert np.array_equal(_anchors_of(dbg, ao, len(a)), a), name
        ao += len(a)
        f, p = O.chain_scores(a)
        ch, sc = O.best_chain(a, f, p)
        assert (r.n_chain, r.chain_score) == (len(ch), sc), name
        assert list(dbg["chain"][co:co + r.n_chain]) == ch, name
        co += r.n_chain
        if r.mapped:
            n_mapped += 1
            _check_record(r, ops, s, seqs[r.ctg])
    assert n_mapped >= 7
    al.close()


# --------------------------------------------------------------------------------------------------------- 3. chain ring

def test_chain_ring_of_64_predecessors():
    """map_chain_kernel: the colinear predecessor 62, 64 (the ring's last lane), 65, 66 and 70 anchors back; ties between
    two identical contigs (the first wins) and between the strands of an inverted repeat (+ wins); chains of exactly 2
    and 3 anchors, chain scores of 39 and 40"""
    names, seqs, _ = E.ring_index()
    idx = E.oracle_index("ring")
    al = _aligner(names, seqs)
    cases = E.ring_reads()
    reads = [s for _, s in cases]
    recs, ops, dbg = al.map_raw(reads, debug=True)
    hits = al.map_batch(reads)
    ao = co = 0
    for i, (name, s) in enumerate(cases):
        r = recs[i]
        a, f, p, ch, sc = E.chain_of(idx, s)
        assert r.n_anchors == len(a) and np.array_equal(_anchors_of(dbg, ao, len(a)), a), name
        ao += len(a)
        assert (r.n_chain, r.chain_score) == (len(ch), sc), name
        assert list(dbg["chain"][co:co + r.n_chain]) == ch, name
        co += r.n_chain
        if len(s) <= 1000:                       # the whole hit too, where the restatement's DP is cheap
            assert hits[i] == O.map_read(idx, s), name
        else:
            assert r.mapped
        if r.mapped:
            _check_record(r, ops, s, seqs[r.ctg])
    by = {name: recs[i] for i, (name, _) in enumerate(cases)}
    assert by["copies_64"].n_chain > 100 and by["copies_65"].n_chain < 50
    assert (by["twin"].mapped, by["twin"].ctg, by["twin"].strand) == (1, 1, 1)
    assert (by["inverted"].mapped, by["inverted"].ctg, by["inverted"].strand) == (1, 3, 1)
    assert by["chain_of_2"].mapped == 0 and by["chain_score_39"].mapped == 0
    assert (by["chain_of_3_mapped"].mapped, by["chain_of_3_mapped"].n_chain) == (1, 3)
    al.close()


# --------------------------------------------------------------------------------------------------------- 4. band

@pytest.fixture(scope="module")
def band_aligner():
    names, seqs, reads = E.band_index()
    al = _aligner(names, seqs)
    yield al
    al.close()


BAND_GROUPS = {
    "ends_and_ties": ("contig_inside_read", "over_left_end", "over_right_end", "short_contig_minus", "tandem_tie",
                      "whole_contig"),
    "deletions": tuple("deletion_%d" % g for g in E.GAP_LENGTHS + (E.GAP_TOO_LONG,)),
    "insertions": tuple("insertion_%d" % g for g in E.GAP_LENGTHS + (E.GAP_TOO_LONG,)),
}


@pytest.mark.parametrize("group", sorted(BAND_GROUPS))
def test_band_masks_shifts_ties_and_traceback(band_aligner, group):
    """map_align_kernel / map_trace_kernel: band starts, score, every hit field and every op byte against the
    restatement, where columns left of the contig and right of it are masked in every row, where the previous row moves
    through LDS by up to some twenty columns a row in either direction, and where best cells tie"""
    names, seqs, cases = E.band_index()
    idx = E.oracle_index("band")
    al = band_aligner
    pick = BAND_GROUPS[group]
    reads = [cases[n][0] for n in pick]
    recs, ops, dbg = al.map_raw(reads, debug=True)
    hits = al.map_batch(reads)
    want = [O.map_read(idx, s, detail=True) for s in reads]
    _check_stages(pick, reads, recs, dbg, want, hits)
    by = {}
    for i, name in enumerate(pick):
        r, (hit, info) = recs[i], want[i]
        assert r.mapped and (r.ctg, r.strand) == cases[name][1:], name
        assert bytes(ops[r.op_off:r.op_off + r.n_ops]) == _ops_of_cs(hit.cs), name
        _check_record(r, ops, reads[i], seqs[r.ctg])
        by[name] = r
    if group == "ends_and_ties":
        r = by["contig_inside_read"]
        assert (r.r_st, r.r_en, r.q_st, r.q_en, r.nm, r.score) == (0, 300, 400, 700, 0, 600)
        assert by["over_left_end"].r_st == 0 and by["over_right_end"].r_en == len(seqs[by["over_right_end"].ctg])
        assert by["short_contig_minus"].r_en - by["short_contig_minus"].r_st > 380
        # the end cells of the two copies tie: the smaller column, so the first copy
        r = by["tandem_tie"]
        assert (r.r_st, r.r_en, r.q_st, r.q_en, r.score) == (0, 200, 0, 200, 400)
        r = by["whole_contig"]
        assert (r.r_st, r.r_en, r.q_st, r.q_en, r.score, r.nm) == (0, 500, 0, 500, 1000, 0)
    else:
        kind = 3 if group == "deletions" else 2
        for g in E.GAP_LENGTHS:              # one hit over both flanks (the band may split the gap's columns in two runs)
            r = by["%s_%d" % (group[:-1], g)]
            n_gap = int((np.asarray(ops[r.op_off:r.op_off + r.n_ops]) == kind).sum())
            assert r.q_en - r.q_st > 3800 and r.r_en - r.r_st > 3800 and n_gap >= g - 20, (g, n_gap)
        r = by["%s_%d" % (group[:-1], E.GAP_TOO_LONG)]    # beyond MAX_DD: one flank
        assert 1900 < r.q_en - r.q_st < 2100 and 1900 < r.r_en - r.r_st < 2100


def test_ops_capacity_one_below_the_need(band_aligner):
    """po_map_batch_h: ops_cap one below the need is E_CAP with the records still written and the need reported; the
    same call at the exact need succeeds"""
    from poreover_amd import _lib
    lib = _lib.load()
    names, seqs, cases = E.band_index()
    reads = [cases[n][0] for n in ("tandem_tie", "short_contig_minus", "whole_contig")]
    full, ops = band_aligner.map_raw(reads)
    need = len(ops)
    assert need == sum(full[i].n_ops for i in range(3)) and all(full[i].mapped for i in range(3))
    buf, off = mapping._pack(reads)
    recs = (mapping.MapHit * 3)()
    small = np.zeros(need - 1, np.uint8)
    got = C.c_int64(0)
    rc = lib.po_map_batch_h(band_aligner._idx, buf.ctypes.data, off.ctypes.data, 3, 0, C.addressof(recs), small.ctypes.data,
                            need - 1, C.byref(got), None, None)
    assert rc == _lib.E_CAP and got.value == need
    assert [t[0] for t in _records(recs, ops, 3)] == [t[0] for t in _records(full, ops, 3)]
    assert not small.any()                                    # nothing is written into a buffer that is too small
    with pytest.raises(_lib.EngineError) as e:
        band_aligner.map_raw(reads, ops_cap=need - 1)
    assert e.value.code == _lib.E_CAP
    exact, ops2 = band_aligner.map_raw(reads, ops_cap=need)
    assert _records(exact, ops2, 3) == _records(full, ops, 3)


# --------------------------------------------------------------------------------------------------------- 5. Gotoh

def test_device_alignment_is_a_plain_gotoh_where_the_band_is_the_matrix():
    """contigs of at most 240 bases and reads of at most 200: every row's 512 columns cover the contig, so the device's
    banded alignment must be a plain affine local alignment: its score the matrix's maximum, its end cell the first
    maximum in row-major order, its op string worth its score"""
    names, seqs, _ = E.gotoh_index()
    cases = E.gotoh_cases()
    al = _aligner(names, seqs)
    reads = [c[0] for c in cases]
    recs, ops = al.map_raw(reads)
    n_mapped = 0
    for i, (rd, c, strand, err) in enumerate(cases):
        r = recs[i]
        Q = O.reverse_complement_q(rd) if strand < 0 else rd
        H = E.gotoh_matrix(O.codes(Q), O.codes(seqs[c]))
        assert r.score == int(H.max()), (i, err)
        assert bool(r.mapped) == (r.score >= O.MIN_SCORE)
        if not r.mapped:
            continue
        n_mapped += 1
        assert (r.ctg, r.strand) == (c, strand)
        y, x = np.unravel_index(int(np.argmax(H)), H.shape)      # the first maximum, rows first
        assert (len(rd) - r.q_st if strand < 0 else r.q_en, r.r_en) == (y, x), (i, err)
        _check_record(r, ops, rd, seqs[c])
    assert n_mapped >= 20
    al.close()


# --------------------------------------------------------------------------------------------------------- 6. pairs

@pytest.fixture(scope="module")
def pairs_run():
    from poreover_amd import _lib
    _lib.load()
    names, targets, queries, cands, tags, plants = E.pairs_set()
    targets, queries = list(targets), list(queries)
    qt = [(q, t) for t, q in cands]
    stats = np.zeros(8)
    recs, ops = mapping.map_pairs_raw(targets, queries, qt, stats=stats)
    return names, targets, queries, cands, tags, plants, qt, _records(recs, ops, len(qt)), stats


def test_pairs_segments_equal_one_contig_indexes(pairs_run):
    """pairs_segsort / pairs_maxocc / pairs_anchor_*: every candidate's record is that of a one-contig index of its target,
    field for field and byte for byte: targets of 4095, 4096 (the last sort in LDS) and 4097 minimizers, of 4999, 5000
    and 5001 distinct hashes (the quantile's rank leaves n - 1), a count at max_occ and one above it, empty and all-N
    targets in the first and last slots and between real ones"""
    names, targets, queries, cands, tags, plants, qt, got, stats = pairs_run
    assert stats[5] == 1 and stats[7] == len(targets)           # one batch: all segments side by side
    planted_anchors = {}
    for i, ((t, q), tag) in enumerate(zip(cands, tags)):
        al = mapping.Aligner.from_sequences([names[t]], [targets[t]])
        recs, ops, dbg = al.map_raw([queries[q]], debug=True)
        assert got[i] == _records(recs, ops, 1, ctg=t)[0], tag
        a = _anchors_of(dbg, 0, recs[0].n_anchors)
        idx = O.Index([names[t]], [targets[t]])
        assert al.max_occ == idx.max_occ and np.array_equal(a, O.anchors(idx, queries[q])), tag
        for k, pos in plants.items():
            if tag.startswith(k.split("_")[0]):
                planted_anchors[(tag, k)] = E.anchors_at(a, pos)
        if recs[0].mapped:
            _check_record(recs[0], ops, queries[q], targets[t])
        al.close()
    # max_occ through its effect: the 15-mer planted 12 times gives anchors up to 5000 distinct hashes and none at 5001;
    # with counts of 11 and 12 and max_occ == 11 the first is kept
    assert planted_anchors == {("distinct_4999", "distinct"): 12, ("distinct_5000", "distinct"): 12,
                               ("distinct_5001", "distinct"): 0, ("boundary", "boundary_kept"): 11,
                               ("boundary", "boundary_dropped"): 0}
    mapped = {tag: got[i][0][0] for i, tag in enumerate(tags) if not tag.endswith("_target")}
    assert all(mapped[t] for t in mapped if not t.startswith("empty")) and not mapped["empty_both"]
    assert not mapped["empty_query"] and not any(got[i][0][0] for i, tag in enumerate(tags) if tag.endswith("_target"))


def test_pairs_equal_the_cpu_restatement(pairs_run):
    """every candidate's Hit is tests/_pairs_oracle.py's: the query mapped by the restatement against its target alone"""
    names, targets, queries, cands, tags, plants, qt, got, stats = pairs_run
    hits = mapping.map_pairs(targets, queries, qt, names=names)
    # the restatement keeps targets and queries in one list
    both = list(targets) + list(queries)
    both_names = list(names) + ["query%d" % k for k in range(len(queries))]
    cache = {}
    for i, ((t, q), h) in enumerate(zip(cands, hits)):
        assert h == PO.map_candidate(both_names, both, t, len(targets) + q, cache), tags[i]
        assert (h is not None) == bool(got[i][0][0])


def test_pairs_shared_target_in_one_batch_and_in_several(pairs_run):
    """two candidates on one target: in the same batch the target's segment is built once, in different batches twice"""
    names, targets, queries, cands, tags, plants, qt, got, stats = pairs_run
    keep = [i for i, tag in enumerate(tags) if tag.startswith(("shared", "empty", "all_n", "minimizers_4097"))]
    sub = [qt[i] for i in keep]
    st = np.zeros(8)
    recs, ops = mapping.map_pairs_raw(targets, queries, sub, stats=st)
    assert st[5] == 1 and st[7] == len({t for _, t in sub})
    assert _records(recs, ops, len(sub)) == [got[i] for i in keep]
    st = np.zeros(8)
    recs, ops = mapping.map_pairs_raw(targets, queries, sub, budget=1, stats=st)          # everyone alone
    assert st[5] == st[7] == len(sub)
    assert _records(recs, ops, len(sub)) == [got[i] for i in keep]
