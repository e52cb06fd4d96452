// pair-decode --skip_matches on the device (pair_decode.py:412-467,512-522): anchors and boxes of every pair's
// alignment, the boxes' rows gathered into a box-major batch for the pair beam search (po_launch_beam2d_geom, as it is), and the
// anchors and box consensuses stitched in signal order.  The rule is po_skip_rules.h's; this file is its wave form and the chain.
//
//   plan:  aln_off | Viterbi x 2, alignment + skips + envelope with the alignment handed out (po_launch_pair_prep_hand) |
//          skip_boxes_kernel | skip_scan_kernel | D2H of the box totals, stream synchronise
//   run:   skip_layout_kernel | skip_gather_kernel | po_launch_beam2d_geom on the boxes | skip_stitch_kernel
#include <algorithm>

#define PO_WANT_ZERO_KERNEL 1
#include "po_device.h"
#include "po_host.h"
#include "po_internal.h"
#include "po_skip_rules.h"

namespace {

struct SkipArgs {
    const char* aln1; const char* aln2; const int64_t* aln_off; const int32_t* ncol; int n;
    const int32_t* map1; const int64_t* map1_off; const int32_t* map2; const int64_t* map2_off;   // frame of every base, pair i at map*_off[i]
    const int32_t* len1; const int32_t* len2;   // bases of the basecalls, or NULL: map*_off[i + 1] - map*_off[i]
    const int32_t* lenU; const int32_t* lenV;   // frames, or NULL: map*_off[i + 1] - map*_off[i] (the chain: maps sit at the reads' rows)
    const int32_t* env; const int64_t* env_off; // 2 ints per frame of read 1, pair i at 2 * env_off[i]
    int matches, indels;
    int32_t* status;                            // in: a pair with a non-zero status is passed over; out
    PoSkipAnchor* anchors; PoSkipBox* boxes;    // rows of pair i: po_skip_table_row
    int32_t* n_anchors; int32_t* n_boxes;
    long long* pinfo;                           // 6 per pair: anchors, boxes, rows of read 1 / read 2 of its boxes, the largest of each
};

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// alignment capacities of the chain: pair i may have U_i + V_i + 16 columns
__global__ __launch_bounds__(64) void skip_aln_off_kernel(const int64_t* y1_off, const int64_t* y2_off, int n, int64_t* aln_off) {
    for (int i = blockIdx.x * 64 + threadIdx.x; i <= n; i += gridDim.x * 64)
        aln_off[i] = (y1_off[i] - y1_off[0]) + (y2_off[i] - y2_off[0]) + 16ll * i;
}

// ---- anchors and boxes: one wave per pair, 64 alignment columns at a time.  Run starts are a ballot of "state differs from the
// previous column, or is mis"; a column that starts a run closes the one before it, whose start is the next lower set bit (or the
// carry); a2s is a popcount prefix of the non-gap ballots; anchors go out in column order by a ballot prefix count.  The four
// a2s values of an anchor wait in its row of the box table until the second pass turns them into boxes.
__global__ __launch_bounds__(64) void skip_boxes_kernel(SkipArgs a) {
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (i >= a.n) return;
    const int64_t row0 = po_skip_table_row(a.aln_off[i], a.aln_off[0], i, a.matches, a.indels);
    const int64_t cap = po_skip_table_row(a.aln_off[i + 1], a.aln_off[0], i + 1, a.matches, a.indels) - 1 - row0;
    PoSkipAnchor* const anc = a.anchors + row0;
    PoSkipBox* const box = a.boxes + row0 + i;
    int st = a.status[i];
    const int ncol = a.ncol[i];
    if (st == PO_OK && (ncol < 1 || ncol > a.aln_off[i + 1] - a.aln_off[i])) st = PO_E_ARG;
    int na = 0;
    if (st == PO_OK) {
        const char* const r1 = a.aln1 + a.aln_off[i];
        const char* const r2 = a.aln2 + a.aln_off[i];
        PoSkipCarry cy = po_skip_carry_init();
        for (int c0 = 0; c0 < ncol; c0 += 64) {
            const int k = c0 + lane;
            const bool in = k < ncol;
            const char x1 = in ? r1[k] : '-', x2 = in ? r2[k] : '-';
            const int s = po_skip_state(x1, x2);
            int ps = __shfl_up(s, 1);
            if (lane == 0) ps = cy.prev_state;
            const unsigned long long S = __ballot(in && po_skip_starts(s, ps));
            const unsigned long long G0 = __ballot(in && x1 != '-'), G1 = __ballot(in && x2 != '-');
            const PoSkipClose c = po_skip_lane_close(c0, lane, S, G0, G1, ps, cy, a.matches, a.indels);
            const unsigned long long R = __ballot(c.rep != 0);
            if (c.rep) {
                const long long idx = na + po_skip_popc(R & po_skip_below(lane));
                if (idx < cap) {
                    anc[idx] = PoSkipAnchor{c.cs, c.ce, c.type, 0};
                    box[idx] = PoSkipBox{c.a0cs, c.a1cs, c.a0ce, c.a1ce};
                }
            }
            na += po_skip_popc(R);
            const int cnt = min(64, ncol - c0);
            cy = po_skip_carry_next(c0, cnt, S, G0, G1, __shfl(s, cnt - 1), cy);
        }
        if (na > cap) st = PO_E_CAP;   // (cannot happen: an anchor has min(matches, indels) columns at least)
        else if (na == 0) st = PO_E_NO_ANCHOR;
    }
    long long r1s = 0, r2s = 0;
    int r1m = 0, r2m = 0;
    if (st == PO_OK) {
        __threadfence();   // the first pass's rows are read back by other lanes
        const int64_t o1 = a.map1_off[i], o2 = a.map2_off[i];
        const int l1 = a.len1 ? a.len1[i] : (int)(a.map1_off[i + 1] - o1), l2 = a.len2 ? a.len2[i] : (int)(a.map2_off[i + 1] - o2);
        const int U = a.lenU ? a.lenU[i] : (int)(a.map1_off[i + 1] - o1), V = a.lenV ? a.lenV[i] : (int)(a.map2_off[i + 1] - o2);
        const int32_t* const env = a.env + 2 * a.env_off[i];
        int carry0 = 0, carry1 = 0, bad = 0;
        for (int k0 = 0; k0 <= na; k0 += 64) {
            const int k = k0 + lane;
            const bool in = k <= na;
            PoSkipBox t = {0, 0, 0, 0};
            if (in && k < na) t = box[k];
            int p0 = __shfl_up(t.lo, 1), p1 = __shfl_up(t.hi, 1);
            if (lane == 0) { p0 = carry0; p1 = carry1; }
            carry0 = __shfl(t.lo, 63); carry1 = __shfl(t.hi, 63);
            int rc = PO_OK;
            if (in) {
                PoSkipBox b;
                int pos;
                rc = po_skip_box(k, na, p0, p1, t.b0, t.b1, a.map1 + o1, l1, a.map2 + o2, l2, U, V, env, &b, &pos);
                box[k] = b;
                if (k < na) anc[k].pos = pos;
                if (rc == PO_OK) {
                    const int rows1 = b.b1 - b.b0, rows2 = max(b.hi - b.lo, 0);
                    r1s += rows1; r2s += rows2; r1m = max(r1m, rows1); r2m = max(r2m, rows2);
                }
            }
            if (__ballot(in && rc != PO_OK)) bad = 1;
        }
        if (bad) st = PO_E_BOX;
    }
    r1s = wave_sum(r1s); r2s = wave_sum(r2s); r1m = wave_max(r1m); r2m = wave_max(r2m);
    if (lane == 0) {
        const bool ok = st == PO_OK;
        long long* const p = a.pinfo + 6ll * i;
        p[0] = (ok || st == PO_E_BOX) ? na : 0; p[1] = ok ? na + 1 : 0;
        p[2] = ok ? r1s : 0; p[3] = ok ? r2s : 0; p[4] = ok ? r1m : 0; p[5] = ok ? r2m : 0;
        a.status[i] = st;
        if (a.n_anchors) a.n_anchors[i] = (int32_t)p[0];
        if (a.n_boxes) a.n_boxes[i] = (int32_t)p[1];
    }
}

// ---- exclusive prefix sums over the pairs of (boxes, rows of read 1, rows of read 2): base[3 i ..], base[3 n ..] = the totals,
// and the largest box.  One workgroup: thread t sums its stretch of pairs, thread 0 the 256 stretches.
__global__ __launch_bounds__(256) void skip_scan_kernel(const long long* pinfo, int n, long long* base, long long* totals) {
    __shared__ long long part[256][3];
    __shared__ int mx[2];
    const int t = (int)threadIdx.x;
    const int per = (n + 255) / 256, lo = min(n, t * per), hi = min(n, lo + per);
    if (t == 0) { mx[0] = 0; mx[1] = 0; }
    __syncthreads();
    long long s[3] = {0, 0, 0};
    int m1 = 0, m2 = 0;
    for (int i = lo; i < hi; ++i) {
        for (int q = 0; q < 3; ++q) s[q] += pinfo[6ll * i + 1 + q];
        m1 = max(m1, (int)pinfo[6ll * i + 4]); m2 = max(m2, (int)pinfo[6ll * i + 5]);
    }
    for (int q = 0; q < 3; ++q) part[t][q] = s[q];
    atomicMax(&mx[0], m1); atomicMax(&mx[1], m2);
    __syncthreads();
    if (t == 0) {
        long long acc[3] = {0, 0, 0};
        for (int u = 0; u < 256; ++u)
            for (int q = 0; q < 3; ++q) { const long long v = part[u][q]; part[u][q] = acc[q]; acc[q] += v; }
        for (int q = 0; q < 3; ++q) { base[3ll * n + q] = acc[q]; totals[q] = acc[q]; }
        totals[3] = mx[0]; totals[4] = mx[1];
    }
    __syncthreads();
    for (int q = 0; q < 3; ++q) s[q] = part[t][q];
    for (int i = lo; i < hi; ++i)
        for (int q = 0; q < 3; ++q) { base[3ll * i + q] = s[q]; s[q] += pinfo[6ll * i + 1 + q]; }
}

struct BoxBatch {   // the box-major batch, in the run workspace
    int64_t* y1_off; int64_t* y2_off; int64_t* seq_off;   // [NB + 1]
    int64_t* src1; int64_t* src2;                         // [NB]: first row of the box in y1 / y2
    int32_t* lo;                                          // [NB]
    int32_t* rowbox1; int32_t* rowbox2;                   // box of every row of the batch
    double* y1; double* y2; int32_t* env;
    char* seq; int32_t* seq_len; int32_t* status;
};
struct PairTabs {   // what the plan left
    const int64_t* aln_off; const char* aln1; const char* aln2;
    const PoSkipAnchor* anchors; const PoSkipBox* boxes; const long long* pinfo; const long long* base;
    int matches, indels;
};

// ---- where every box sits in the batch: one wave per pair, an exclusive scan over its boxes
__global__ __launch_bounds__(64) void skip_layout_kernel(PairTabs p, int n, const int64_t* y1_off, const int64_t* y2_off, BoxBatch b) {
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (i >= n) return;
    if (i == 0 && lane == 0) {
        const long long NB = p.base[3ll * n], T1 = p.base[3ll * n + 1], T2 = p.base[3ll * n + 2];
        b.y1_off[NB] = T1; b.y2_off[NB] = T2; b.seq_off[NB] = T1 + T2;
    }
    const int nb = (int)p.pinfo[6ll * i + 1];
    if (nb == 0) return;
    const PoSkipBox* const box = p.boxes + po_skip_table_row(p.aln_off[i], p.aln_off[0], i, p.matches, p.indels) + i;
    const long long bb = p.base[3ll * i];
    long long c1 = p.base[3ll * i + 1], c2 = p.base[3ll * i + 2];
    for (int k0 = 0; k0 < nb; k0 += 64) {
        const int k = k0 + lane;
        PoSkipBox x = {0, 0, 0, 0};
        if (k < nb) x = box[k];
        const int rows1 = x.b1 - x.b0, rows2 = max(x.hi - x.lo, 0);
        int e1 = rows1, e2 = rows2;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t1 = __shfl_up(e1, o), t2 = __shfl_up(e2, o);
            if (lane >= o) { e1 += t1; e2 += t2; }
        }
        const long long f1 = c1 + e1 - rows1, f2 = c2 + e2 - rows2;   // first rows of box k in the batch
        if (k < nb) {
            b.y1_off[bb + k] = f1; b.y2_off[bb + k] = f2; b.seq_off[bb + k] = f1 + f2;
            b.src1[bb + k] = y1_off[i] + x.b0; b.src2[bb + k] = y2_off[i] + x.lo; b.lo[bb + k] = x.lo;
        }
        for (int q = 0; q < min(64, nb - k0); ++q) {
            const long long g1 = __shfl(f1, q), g2 = __shfl(f2, q);
            const int n1 = __shfl(rows1, q), n2 = __shfl(rows2, q);
            for (int r = lane; r < n1; r += 64) b.rowbox1[g1 + r] = (int32_t)(bb + k0 + q);
            for (int r = lane; r < n2; r += 64) b.rowbox2[g2 + r] = (int32_t)(bb + k0 + q);
        }
        c1 += __shfl(e1, 63); c2 += __shfl(e2, 63);
    }
}

// ---- the boxes' rows of y1 and y2 and their shifted envelope rows, box-major: flat over 8-byte elements (a double of a
// table, or the two ints of an envelope row), consecutive lanes on consecutive elements of a row
__global__ __launch_bounds__(256) void skip_gather_kernel(const double* y1, const double* y2, const int32_t* env, int C, long long T1, long long T2,
                                                          BoxBatch b) {
    const long long E1 = T1 * C, E2 = T2 * C, E = E1 + E2 + T1;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        if (e < E1) {
            const long long row = e / C;
            const int c = (int)(e - row * C), j = b.rowbox1[row];
            b.y1[e] = y1[(b.src1[j] + (row - b.y1_off[j])) * C + c];
        } else if (e < E1 + E2) {
            const long long f = e - E1, row = f / C;
            const int c = (int)(f - row * C), j = b.rowbox2[row];
            b.y2[f] = y2[(b.src2[j] + (row - b.y2_off[j])) * C + c];
        } else {
            const long long row = e - E1 - E2;
            const int j = b.rowbox1[row];
            const int2 v = ((const int2*)env)[b.src1[j] + (row - b.y1_off[j])];
            ((int2*)b.env)[row] = make_int2(v.x - b.lo[j], v.y - b.lo[j]);
        }
    }
}

// ---- a pair's consensus: box 0, anchor 0, box 1, ..., box na (the join order of po_skip_rules.h).  One wave per pair: the
// boxes' statuses and the sum of the piece lengths first, then the pieces one after the other at a running offset.
__global__ __launch_bounds__(64) void skip_stitch_kernel(PairTabs p, int n, BoxBatch b, char* seq, const int64_t* seq_off, int32_t* seq_len,
                                                         int32_t* status) {
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (i >= n) return;
    if (status[i] != PO_OK) { if (lane == 0) seq_len[i] = 0; return; }
    const int64_t row0 = po_skip_table_row(p.aln_off[i], p.aln_off[0], i, p.matches, p.indels);
    const PoSkipAnchor* const anc = p.anchors + row0;
    const PoSkipBox* const box = p.boxes + row0 + i;
    const int na = (int)p.pinfo[6ll * i], nb = na + 1;
    const long long bb = p.base[3ll * i];
    long long total = 0;
    int first_bad = PO_OK;
    for (int k0 = 0; k0 < nb; k0 += 64) {
        const int k = k0 + lane;
        const int bs = k < nb ? b.status[bb + k] : PO_OK;
        if (k < nb && bs == PO_OK) total += b.seq_len[bb + k];
        if (k < na) total += anc[k].ce - anc[k].cs;
        const unsigned long long m = __ballot(bs != PO_OK);
        if (m && first_bad == PO_OK) first_bad = __shfl(bs, __builtin_ctzll(m));
    }
    total = wave_sum(total);
    const long long room = seq_off[i + 1] - seq_off[i];
    if (first_bad != PO_OK || total > room) {
        if (lane == 0) { status[i] = first_bad != PO_OK ? first_bad : PO_E_CAP; seq_len[i] = 0; }
        return;
    }
    char* const out = seq + seq_off[i];
    const char* const r1 = p.aln1 + p.aln_off[i];
    const char* const r2 = p.aln2 + p.aln_off[i];
    long long off = 0;
    auto put = [&](const char* src, int len) {
        for (int c = lane; c < len; c += 64) out[off + c] = src[c];
        off += len;
    };
    bool early = false;   // box k went out before anchor k - 1 (the tie)
    for (int k = 0; k < nb; ++k) {
        if (!early) put(b.seq + b.seq_off[bb + k], b.seq_len[bb + k]);
        early = false;
        if (k < na) {
            const PoSkipAnchor an = anc[k];
            const char* const text = (an.type == PO_SKIP_INS ? r2 : r1) + an.cs;
            const char* const nxt = b.seq + b.seq_off[bb + k + 1];
            const int nlen = b.seq_len[bb + k + 1];
            if (box[k + 1].b0 == an.pos && po_skip_text_less(nxt, nlen, text, an.ce - an.cs)) { put(nxt, nlen); early = true; }
            put(text, an.ce - an.cs);
        }
    }
    if (lane == 0) seq_len[i] = (int32_t)total;
}

// ---- workspaces
struct PlanGeom {
    size_t off_pp, pp_bytes, off_aln_off, off_aln1, off_aln2, off_ncol, off_anc, off_box, off_pinfo, off_base, off_totals, off_env, total;
    int64_t aln_bytes, tab_rows;
};
PlanGeom plan_geometry(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, const po_pair_options* opt, int matches, int indels) {
    PlanGeom g;
    const size_t np = (size_t)(n > 0 ? n : 1);
    g.aln_bytes = tr1 + tr2 + 16ll * n;
    g.tab_rows = po_skip_table_row(g.aln_bytes, 0, n, matches, indels);
    size_t o = 0;
    g.off_pp = o; g.pp_bytes = po_pair_ws_bytes_impl(n, tr1, tr2, mr1, mr2, C, opt); o += al256(g.pp_bytes);
    g.off_aln_off = o; o += al256(sizeof(int64_t) * (np + 1));
    g.off_aln1 = o; o += al256((size_t)g.aln_bytes);
    g.off_aln2 = o; o += al256((size_t)g.aln_bytes);
    g.off_ncol = o; o += al256(sizeof(int32_t) * np);
    g.off_anc = o; o += al256(sizeof(PoSkipAnchor) * (size_t)(g.tab_rows + 1));
    g.off_box = o; o += al256(sizeof(PoSkipBox) * (size_t)(g.tab_rows + n + 1));
    g.off_pinfo = o; o += al256(sizeof(long long) * 6 * np);
    g.off_base = o; o += al256(sizeof(long long) * 3 * (np + 1));
    g.off_totals = o; o += 256;
    g.off_env = o; o += al256(sizeof(int32_t) * 2 * (size_t)tr1);
    g.total = o + 256;
    return g;
}
PairTabs plan_tabs(char* w, const PlanGeom& g, int matches, int indels) {
    PairTabs p;
    p.aln_off = (const int64_t*)(w + g.off_aln_off); p.aln1 = w + g.off_aln1; p.aln2 = w + g.off_aln2;
    p.anchors = (const PoSkipAnchor*)(w + g.off_anc); p.boxes = (const PoSkipBox*)(w + g.off_box);
    p.pinfo = (const long long*)(w + g.off_pinfo); p.base = (const long long*)(w + g.off_base);
    p.matches = matches; p.indels = indels;
    return p;
}

struct RunGeom {
    size_t off_y1o, off_y2o, off_so, off_src1, off_src2, off_lo, off_st, off_len, off_rb1, off_rb2, off_y1, off_y2, off_env, off_seq, off_b2,
        b2_bytes, total;
};
RunGeom run_geometry(int C, const po_pair_options* opt, const po_skip_totals* t) {
    RunGeom g;
    const size_t NB = (size_t)std::max<int64_t>(t->n_boxes, 1), T1 = (size_t)std::max<int64_t>(t->total_rows1, 1),
                 T2 = (size_t)std::max<int64_t>(t->total_rows2, 1);
    size_t o = 0;
    g.off_y1o = o; o += al256(8 * (NB + 1));
    g.off_y2o = o; o += al256(8 * (NB + 1));
    g.off_so = o; o += al256(8 * (NB + 1));
    g.off_src1 = o; o += al256(8 * NB);
    g.off_src2 = o; o += al256(8 * NB);
    g.off_lo = o; o += al256(4 * NB);
    g.off_st = o; o += al256(4 * NB);
    g.off_len = o; o += al256(4 * NB);
    g.off_rb1 = o; o += al256(4 * T1);
    g.off_rb2 = o; o += al256(4 * T2);
    g.off_y1 = o; o += al256(8 * T1 * (size_t)C);
    g.off_y2 = o; o += al256(8 * T2 * (size_t)C);
    g.off_env = o; o += al256(8 * T1);
    g.off_seq = o; o += al256(T1 + T2);
    g.off_b2 = o;
    g.b2_bytes = po_beam2d_ws_bytes_impl((int)NB, t->total_rows1, t->total_rows2, t->max_rows1, t->max_rows2, C, opt->beam_width, opt->model,
                                         opt->method);
    o += al256(g.b2_bytes);
    g.total = o + 256;
    return g;
}

int check_options(int C, const po_pair_options* opt, int matches, int indels) {
    if (!opt || matches < 1 || indels < 1) return PO_E_ARG;
    if (opt->model < 0 || opt->model > 2) return PO_E_ARG;
    if ((opt->model == PO_MODEL_FLIPFLOP) ? (C != 2 * PO_A) : (C != PO_A + 1)) return PO_E_ARG;
    if (opt->diagonal_envelope) return PO_E_UNSUPPORTED;
    return PO_OK;
}

}  // namespace

extern "C" size_t po_skip_plan_ws_bytes(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, const po_pair_options* opt,
                                        int matches, int indels) {
    if (check_options(C, opt, matches, indels) != PO_OK) return 0;
    return plan_geometry(n, tr1, tr2, mr1, mr2, C, opt, matches, indels).total;
}

extern "C" int po_launch_skip_plan(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                                   const po_pair_options* opt, int matches, int indels, int64_t tr1, int64_t tr2, int64_t mr1,
                                   int64_t mr2, char* seq1d, const int64_t* seq1d_off, int32_t* len1, int32_t* len2, double* identity,
                                   int32_t* status, int32_t* n_anchors, int32_t* n_boxes, void* ws, size_t ws_bytes,
                                   po_skip_totals* totals, hipStream_t stream) {
    if (totals) *totals = po_skip_totals{0, 0, 0, 0, 0};
    if (n <= 0) return PO_OK;
    int rc = check_options(C, opt, matches, indels);
    if (rc != PO_OK) return rc;
    if (!totals) return PO_E_ARG;
    const PlanGeom g = plan_geometry(n, tr1, tr2, mr1, mr2, C, opt, matches, indels);
    if (ws_bytes < g.total) return PO_E_CAP;
    char* const w = (char*)ws;
    int64_t* const aln_off = (int64_t*)(w + g.off_aln_off);
    hipLaunchKernelGGL(skip_aln_off_kernel, dim3(std::min(n / 64 + 1, 1024)), dim3(64), 0, stream, y1_off, y2_off, n, aln_off);
    SkipArgs a = {};
    a.aln1 = w + g.off_aln1; a.aln2 = w + g.off_aln2; a.aln_off = aln_off; a.ncol = (int32_t*)(w + g.off_ncol); a.n = n;
    const int32_t* env = nullptr;
    rc = po_launch_pair_prep_hand(y1, y1_off, y2, y2_off, n, C, opt, tr1, tr2, mr1, mr2, seq1d, seq1d_off, len1, len2, identity,
                                  (int32_t*)(w + g.off_env), status, w + g.off_aln1, w + g.off_aln2, aln_off, (int32_t*)(w + g.off_ncol),
                                  &a.map1, &a.map2, &env, w + g.off_pp, g.pp_bytes, stream);
    if (rc != PO_OK) return rc;
    a.map1_off = y1_off; a.map2_off = y2_off; a.len1 = len1; a.len2 = len2;
    a.env = env; a.env_off = y1_off;
    a.matches = matches; a.indels = indels; a.status = status;
    a.anchors = (PoSkipAnchor*)(w + g.off_anc); a.boxes = (PoSkipBox*)(w + g.off_box);
    a.n_anchors = n_anchors; a.n_boxes = n_boxes; a.pinfo = (long long*)(w + g.off_pinfo);
    hipLaunchKernelGGL(skip_boxes_kernel, dim3(n), dim3(64), 0, stream, a);
    long long* const dev_totals = (long long*)(w + g.off_totals);
    hipLaunchKernelGGL(skip_scan_kernel, dim3(1), dim3(256), 0, stream, a.pinfo, n, (long long*)(w + g.off_base), dev_totals);
    long long h[5];
    if (hipMemcpyAsync(h, dev_totals, sizeof(h), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return PO_E_HIP;
    *totals = po_skip_totals{h[0], h[1], h[2], h[3], h[4]};
    return PO_OK;
}

extern "C" size_t po_skip_run_ws_bytes(int n, int C, const po_pair_options* opt, const po_skip_totals* totals) {
    (void)n;
    if (!opt || !totals) return 0;
    return run_geometry(C, opt, totals).total;
}

// ev (or NULL): four events recorded at the start and after gather, beam and stitch
extern "C" int po_launch_skip_run(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                                  const po_pair_options* opt, int matches, int indels, int64_t tr1, int64_t tr2, int64_t mr1,
                                  int64_t mr2, const po_skip_totals* totals, void* plan_ws, size_t plan_ws_bytes, char* seq,
                                  const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes,
                                  hipEvent_t* ev, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    int rc = check_options(C, opt, matches, indels);
    if (rc != PO_OK) return rc;
    if (!totals || totals->n_boxes < 0 || totals->n_boxes > 0x7fffffff) return PO_E_ARG;
    const PlanGeom pg = plan_geometry(n, tr1, tr2, mr1, mr2, C, opt, matches, indels);
    if (plan_ws_bytes < pg.total) return PO_E_CAP;
    const RunGeom g = run_geometry(C, opt, totals);
    if (ws_bytes < g.total) return PO_E_CAP;
    char* const w = (char*)ws;
    const PairTabs p = plan_tabs((char*)plan_ws, pg, matches, indels);
    BoxBatch b;
    b.y1_off = (int64_t*)(w + g.off_y1o); b.y2_off = (int64_t*)(w + g.off_y2o); b.seq_off = (int64_t*)(w + g.off_so);
    b.src1 = (int64_t*)(w + g.off_src1); b.src2 = (int64_t*)(w + g.off_src2); b.lo = (int32_t*)(w + g.off_lo);
    b.rowbox1 = (int32_t*)(w + g.off_rb1); b.rowbox2 = (int32_t*)(w + g.off_rb2);
    b.y1 = (double*)(w + g.off_y1); b.y2 = (double*)(w + g.off_y2); b.env = (int32_t*)(w + g.off_env);
    b.seq = w + g.off_seq; b.seq_len = (int32_t*)(w + g.off_len); b.status = (int32_t*)(w + g.off_st);
    const int NB = (int)totals->n_boxes;
    const long long T1 = totals->total_rows1, T2 = totals->total_rows2;
    if (ev && hipEventRecord(ev[0], stream) != hipSuccess) return PO_E_HIP;
    if (NB > 0) {
        hipLaunchKernelGGL(skip_layout_kernel, dim3(n), dim3(64), 0, stream, p, n, y1_off, y2_off, b);
        const long long E = (T1 + T2) * C + T1;
        const int blocks = (int)std::min<long long>((E + 255) / 256, (long long)po_dev_info().cus * 16);
        hipLaunchKernelGGL(skip_gather_kernel, dim3(std::max(blocks, 1)), dim3(256), 0, stream, y1, y2,
                           (const int32_t*)((char*)plan_ws + pg.off_env), C, T1, T2, b);
    }
    if (ev && hipEventRecord(ev[1], stream) != hipSuccess) return PO_E_HIP;
    if (NB > 0) {
        const uint32_t alphabet = 'A' | ('C' << 8) | ('G' << 16) | ((uint32_t)'T' << 24);
        rc = po_launch_beam2d_geom(b.y1, b.y1_off, b.y2, b.y2_off, b.env, NB, C, PO_A, alphabet, opt->beam_width, opt->model, opt->method,
                                   T1, T2, totals->max_rows1, totals->max_rows2, b.seq, b.seq_off, b.seq_len, b.status, 0, w + g.off_b2,
                                   g.b2_bytes, stream);
        if (rc != PO_OK) return rc;
    }
    if (ev && hipEventRecord(ev[2], stream) != hipSuccess) return PO_E_HIP;
    hipLaunchKernelGGL(skip_stitch_kernel, dim3(n), dim3(64), 0, stream, p, n, b, seq, seq_off, seq_len, status);
    if (ev && hipEventRecord(ev[3], stream) != hipSuccess) return PO_E_HIP;
    return hipGetLastError() == hipSuccess ? PO_OK : PO_E_HIP;
}

// where the plan's tables are (the host twins copy them out): anchors / boxes int32 x 4 per row, env 2 ints per frame of read 1
extern "C" int po_skip_plan_tables(void* plan_ws, int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C,
                                   const po_pair_options* opt, int matches, int indels, const int32_t** anchors, const int32_t** boxes,
                                   const int32_t** env, int64_t* tab_rows) {
    const int rc = check_options(C, opt, matches, indels);
    if (rc != PO_OK) return rc;
    const PlanGeom g = plan_geometry(n, tr1, tr2, mr1, mr2, C, opt, matches, indels);
    char* const w = (char*)plan_ws;
    *anchors = (const int32_t*)(w + g.off_anc); *boxes = (const int32_t*)(w + g.off_box); *env = (const int32_t*)(w + g.off_env);
    *tab_rows = g.tab_rows;
    return PO_OK;
}

// the anchor / box stage on given alignments (po_skip_boxes_batch_h): every pointer a device pointer, status zeroed by the caller,
// pinfo 6 long long per pair of scratch
extern "C" int po_launch_skip_boxes(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol, int n,
                                    const int32_t* map1, const int64_t* map1_off, const int32_t* map2, const int64_t* map2_off,
                                    const int32_t* U, const int32_t* V, const int32_t* env, const int64_t* env_off, int matches,
                                    int indels, int32_t* n_anchors, int32_t* n_boxes, int32_t* anchors, int32_t* boxes,
                                    int32_t* status, long long* pinfo, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    if (matches < 1 || indels < 1) return PO_E_ARG;
    SkipArgs a = {};
    a.aln1 = aln1; a.aln2 = aln2; a.aln_off = aln_off; a.ncol = ncol; a.n = n;
    a.map1 = map1; a.map1_off = map1_off; a.map2 = map2; a.map2_off = map2_off; a.lenU = U; a.lenV = V;
    a.env = env; a.env_off = env_off; a.matches = matches; a.indels = indels; a.status = status;
    a.anchors = (PoSkipAnchor*)anchors; a.boxes = (PoSkipBox*)boxes; a.n_anchors = n_anchors; a.n_boxes = n_boxes; a.pinfo = pinfo;
    hipLaunchKernelGGL(skip_boxes_kernel, dim3(n), dim3(64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? PO_OK : PO_E_HIP;
}
