// `pair-basecall`: scaled signals and a list of read pairs in, 1D² consensus strings out, in one device-resident pass
// (DESIGN.md §17).
//
// What `call` followed by `pair-decode` does in two commands and a file per read — the network's forward pass (po_call.hip),
// the log-softmax of its logits with read 2's time reversal and column permutation (po_ingest.hip) and the pair chain
// (po_pair.hip: Viterbi of both reads, length skip, alignment, identity skip, envelope, pair beam search) — with the
// per-frame data staying on the device in between and with `basecall`'s overlapping windows (po_basecall_pass.h: the same
// pass loop, so a window's logits are the same bits).
//
//   pair_table_kernel   the stitched logits (read-major f32) to the two pair-major f64 log-probability tables that
//                       po_pair_decode_batch reads; a read may stand in several pairs and on either side
//
// A streaming copy like ingest_kernel: one lane per output frame, 20 bytes in, 40 bytes out, a frame's five values
// contiguous on both sides; every output value has one writer, so two runs give the same bits.
//
// po_pair_basecall_fastq_batch_h is the same body followed by the quality stages on the same stream:
// PairFastqStages below enqueues them (kernels: po_fastq.hip, the lattice: po_qual.hip) on the two tables, the 1-D strings
// and the consensus the pair chain left on the device.  po_pair_qual_h runs those stages alone on host buffers.
#include <algorithm>
#include <cstring>
#include <string>

#include "po_basecall_pass.h"
#include "po_fastq_rules.h"
#include "po_fastq_stages.h"
#include "po_ingest_rules.h"
#include "po_pair_basecall_pass.h"
#include "po_pair_basecall_plan.h"
#include "po_pair_fastq_plan.h"

namespace {

constexpr int NOUT = 5;   // Dense outputs (A, C, G, T, blank)

struct PTArgs {
    const float* logits;        // [rows of all reads][NOUT], read-major
    const int64_t* sig_off;     // [n_reads + 1] row offsets of the reads
    const int32_t* pair_idx;    // [2 * n_pairs]
    const int64_t* y_off[2];    // [n_pairs + 1] each
    double* y[2];
    int64_t rows0, total;       // rows of table 0, rows of both
    int n_pairs, reverse2;
    int perm2[NOUT];
};

// y[side][row][c] = log-softmax(logits[source row])[c'] with c' = c (side 0) or perm2[c] (side 1); lanes [0, rows0) make
// table 0, lanes [rows0, total) table 1 (po_pair_basecall_plan.h: the source row)
__global__ __launch_bounds__(64) void pair_table_kernel(PTArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * blockDim.x) {
        const int side = i >= a.rows0 ? 1 : 0;
        const int64_t row = side ? i - a.rows0 : i;
        const int64_t src = po_pair_table_source(a.sig_off, a.pair_idx, a.y_off[side], a.n_pairs, side, a.reverse2, row, nullptr);
        double v[NOUT];
        po_ingest_log_softmax_f32(a.logits + src * NOUT, NOUT, v);
        double* o = a.y[side] + row * NOUT;
#pragma unroll
        for (int c = 0; c < NOUT; ++c) {   // (selects, not an indexed read of v: the five values stay in registers)
            const int p = side ? a.perm2[c] : c;
            o[c] = p == 0 ? v[0] : p == 1 ? v[1] : p == 2 ? v[2] : p == 3 ? v[3] : v[4];
        }
    }
}

// the plan's two tables on the device, and the launch
struct PairTables {
    PoDev idx, off[2], y[2];
    int up(const PoPairBasecallPlan& pp, const int32_t* pair_idx_h, int n_pairs) {
        PO_HIPCHK(idx.up(pair_idx_h, sizeof(int32_t) * 2 * (size_t)n_pairs));
        for (int s = 0; s < 2; ++s) {
            PO_HIPCHK(off[s].up(pp.y_off[s].data(), sizeof(int64_t) * pp.y_off[s].size()));
            PO_HIPCHK(y[s].up(nullptr, sizeof(double) * NOUT * (size_t)pp.rows[s]));
        }
        return PO_OK;
    }
    int launch(const PoPairBasecallPlan& pp, const float* logits, const int64_t* sig_off, int n_pairs, int reverse2, const int* perm2,
               hipStream_t stream) {
        PTArgs a;
        a.logits = logits; a.sig_off = sig_off; a.pair_idx = idx;
        for (int s = 0; s < 2; ++s) { a.y_off[s] = off[s]; a.y[s] = y[s]; }
        a.rows0 = pp.rows[0]; a.total = pp.rows[0] + pp.rows[1];
        a.n_pairs = n_pairs; a.reverse2 = reverse2 ? 1 : 0;
        for (int c = 0; c < NOUT; ++c) a.perm2[c] = perm2 ? perm2[c] : c;
        if (a.total <= 0) return PO_OK;
        const int64_t blocks = std::min<int64_t>((a.total + 63) / 64, 256 * 32);
        hipLaunchKernelGGL(pair_table_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, a);
        PO_HIPCHK(hipGetLastError());
        return PO_OK;
    }
};

typedef PoPairBasecallFastq PairFastqOut;

// what the quality stages read: the two tables and the strings on the device, the strings' offset tables on both sides
struct PairQualIn {
    const double* y[2]; const int64_t* y_off[2];   // device
    int64_t rows[2], max_rows[2];
    int n, model;
    const char* seq1d; const int64_t* seq1d_off_h;                      // device; host, 2 n + 1 entries
    const char* seq; const int64_t* seq_off; const int64_t* seq_off_h;  // device; device; host, n + 1 entries
};

int null_quality_pointer(const std::string& me, const PairFastqOut& fq) {
    if (fq.qual1d_h && fq.qual_h && fq.qual_status_h) return PO_OK;
    return po_fail(PO_E_ARG, me + "null argument " + (!fq.qual1d_h ? "qual1d_h" : !fq.qual_h ? "qual_h" : "qual_status_h"));
}

// The quality stages of a pair call, enqueued behind the pair chain on its stream.  The tables, the 1-D
// strings and the consensus stay where they are; lengths, statuses, modes and offsets are the only words that cross.
// Item k of a pair (po_pair_fastq_plan.h) is scored on the table of side s = k & 1; per side there is one Viterbi call
// with its map and one consumed table, which the side's two items use one after the other.
struct PairFastqStages {
    PoDev vseq[2], vlen[2], vst[2], map[2], consumed[2], wsv, mode, guide[PO_PQ_ITEMS];
    PoDev off1d[2], elen[PO_PQ_ITEMS], lob[PO_PQ_ITEMS], lou[PO_PQ_ITEMS], pos[2], sel[2], coff;
    PoDev labels[PO_PQ_ITEMS], odds[PO_PQ_ITEMS], qst[PO_PQ_ITEMS], logp, wsq, qual1d, qual;
    PoFqAligner al;
    PoPairFastqPlan plan;
    size_t s1b = 0, cap = 0, wvb = 0;
    bool banded = false;
    int kind = PO_KIND_POREOVER;
    int qual_route = PO_QUAL_ROUTE_GENERAL;   // the lattices' kernels: po_qual_batch's (po_pair_qual: po_qual_entry_route())

    // before the decoder: the buffers whose size is known from the tables
    int prepare(const PairQualIn& in, const PairFastqOut& fq) {
        const int n = in.n;
        al.reset();   // (a resident state: the pairs of the call before are not this call's)
        wvb = 0;
        banded = fq.band_size > 0;
        kind = in.model == PO_MODEL_MERGE ? PO_KIND_BONITO : PO_KIND_POREOVER;
        s1b = (size_t)in.seq1d_off_h[2 * (size_t)n];
        cap = (size_t)in.seq_off_h[n];
        PO_HIPCHK(qual1d.up(nullptr, s1b));
        PO_HIPCHK(qual.up(nullptr, cap));
        PO_HIPCHK(logp.up(nullptr, sizeof(double) * n));
        if (!banded) return PO_OK;
        PO_HIPCHK(mode.up(nullptr, sizeof(int32_t) * PO_PQ_ITEMS * (size_t)n));
        for (int s = 0; s < 2; ++s) {
            PO_HIPCHK(vseq[s].up(nullptr, (size_t)in.rows[s]));
            PO_HIPCHK(vlen[s].up(nullptr, sizeof(int32_t) * n));
            PO_HIPCHK(vst[s].up(nullptr, sizeof(int32_t) * n));
            PO_HIPCHK(map[s].up(nullptr, sizeof(int32_t) * (size_t)in.rows[s]));
            PO_HIPCHK(consumed[s].up(nullptr, sizeof(int32_t) * (size_t)in.rows[s]));
            wvb = std::max(wvb, po_viterbi_workspace_bytes(n, in.rows[s], NOUT, kind));
        }
        for (int k = 0; k < PO_PQ_ITEMS; ++k) PO_HIPCHK(guide[k].up(nullptr, sizeof(int32_t) * (size_t)in.rows[po_pq_side(k)]));
        PO_HIPCHK(wsv.up(nullptr, wvb));
        return PO_OK;
    }

    // step 1: the Viterbi call of either table with its frame map (the pair chain does not expose its own); a call's string
    // has its table's row offsets: a base per frame at most
    int viterbi(const PairQualIn& in, hipStream_t stream) {
        PO_HIPCHK(hipMemsetAsync(qual1d.p, 0, std::max<size_t>(s1b, 1), stream));
        PO_HIPCHK(hipMemsetAsync(qual.p, 0, std::max<size_t>(cap, 1), stream));
        for (int s = 0; banded && s < 2; ++s) {
            const int rc = po_viterbi_batch(in.y[s], in.y_off[s], in.n, NOUT, "ACGT", kind, nullptr, vseq[s], in.y_off[s], vlen[s], map[s],
                                            vst[s], wsv, wvb, stream);
            if (rc != PO_OK) return rc;
        }
        return PO_OK;
    }

    const char* scored(const PairQualIn& in, int k) const { return k < 2 ? in.seq1d : in.seq; }
    const int64_t* scored_off(const PairQualIn& in, int k) const { return k < 2 ? off1d[k].as<int64_t>() : in.seq_off; }

    // steps 2 and 3, after the pair chain's lengths and statuses have come down: the plan of the four items, the items that
    // need an alignment (one band for all of them, both sides together), the guides
    int guides(const char* me, const PairQualIn& in, const PairFastqOut& fq, const int32_t* st_h, const int32_t* l1_h,
               const int32_t* l2_h, const int32_t* ln_h, hipStream_t stream) {
        const int n = in.n;
        po_pair_fastq_make_plan(in.seq1d_off_h, n, st_h, l1_h, l2_h, ln_h, fq.band_size, fq.unbanded_h, &plan);
        for (int s = 0; s < 2; ++s) {
            PO_HIPCHK(off1d[s].up(plan.off1d[s].data(), sizeof(int64_t) * ((size_t)n + 1)));
            PO_HIPCHK(pos[s].up(plan.pos[2 + s].data(), sizeof(int64_t) * n));
            PO_HIPCHK(sel[s].up(plan.sel[2 + s].data(), sizeof(int32_t) * n));
        }
        PO_HIPCHK(coff.up(plan.cons_off.data(), sizeof(int64_t) * ((size_t)n + 1)));
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {
            PO_HIPCHK(elen[k].up(plan.len_b[k].data(), sizeof(int32_t) * n));
            PO_HIPCHK(lob[k].up(plan.off_b[k].data(), sizeof(int64_t) * ((size_t)n + 1)));
            PO_HIPCHK(lou[k].up(plan.off_u[k].data(), sizeof(int64_t) * ((size_t)n + 1)));
        }
        if (!banded) return PO_OK;
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {
            const int s = po_pq_side(k);
            po_launch_fastq_mode2(scored(in, k), scored_off(in, k), elen[k], vseq[s], in.y_off[s], vlen[s], vst[s], n,
                                  mode.as<int32_t>() + (size_t)k * n, stream);
            PO_HIPCHK(hipGetLastError());
        }
        std::vector<int32_t> h((PO_PQ_ITEMS + 2) * (size_t)n);   // modes of the four item types | called lengths of the two sides
        PO_HIPCHK(hipMemcpyAsync(h.data(), mode.p, sizeof(int32_t) * PO_PQ_ITEMS * n, hipMemcpyDeviceToHost, stream));
        for (int s = 0; s < 2; ++s)
            PO_HIPCHK(hipMemcpyAsync(h.data() + (PO_PQ_ITEMS + s) * (size_t)n, vlen[s].p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipStreamSynchronize(stream));
        int first[PO_PQ_ITEMS + 1] = {0, 0, 0, 0, 0};   // the aligned pairs of item type k: first[k] .. first[k + 1]
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {
            for (int i = 0; i < n; ++i)
                if (h[(size_t)k * n + i] == PO_FQ_ALIGN) al.add(i, h[(PO_PQ_ITEMS + po_pq_side(k)) * (size_t)n + i], plan.len_b[k][i]);
            first[k + 1] = al.m();
        }
        int rc;
        if (al.m() > 0) {
            rc = al.up(me);
            if (rc != PO_OK) return rc;
            for (int k = 0; k < PO_PQ_ITEMS; ++k) {
                const int s = po_pq_side(k), a0 = first[k], mk = first[k + 1] - a0;
                if (mk == 0) continue;
                const int64_t base = al.so[2 * (size_t)a0];
                po_launch_fastq_gather2(vseq[s], in.y_off[s], scored(in, k), scored_off(in, k), al.pair_read.as<int32_t>() + a0,
                                        al.pair_off.as<int64_t>() + 2 * a0, 2 * mk, base, al.so[2 * (size_t)first[k + 1]] - base,
                                        al.pair_seq, stream);
                PO_HIPCHK(hipGetLastError());
            }
            rc = al.run(stream);
            if (rc != PO_OK) return rc;
        }
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {   // (a side's two items use its consumed table one after the other)
            const int s = po_pq_side(k), a0 = first[k], mk = first[k + 1] - a0;
            int32_t* md = mode.as<int32_t>() + (size_t)k * n;
            if (mk > 0) {
                po_launch_fastq_consumed(al.aln1, al.aln2, al.aln_off.as<int64_t>() + a0, al.ncol.as<int32_t>() + a0,
                                         al.ast.as<int32_t>() + a0, mk, al.pair_read.as<int32_t>() + a0, in.y_off[s], vlen[s], elen[k],
                                         consumed[s], md, stream);
                PO_HIPCHK(hipGetLastError());
            }
            po_launch_fastq_guide(map[s], consumed[s], in.y_off[s], n, in.rows[s], vlen[s], elen[k], md, guide[k], stream);
            PO_HIPCHK(hipGetLastError());
        }
        return PO_OK;
    }

    // steps 4 to 6: dense labels, the four items' lattices on the resident tables (an item in the banded call or in the
    // one without a band, L = 0 in the other), Phred characters at the strings' offsets
    int lattice(const PairQualIn& in, const PairFastqOut& fq, hipStream_t stream) {
        const int n = in.n;
        size_t wqb = 0;
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {
            const int s = po_pq_side(k);
            const size_t tot = (size_t)plan.total(k);
            PO_HIPCHK(labels[k].up(nullptr, tot));
            PO_HIPCHK(odds[k].up(nullptr, sizeof(double) * 5 * tot));
            PO_HIPCHK(qst[k].up(nullptr, sizeof(int32_t) * 2 * (size_t)n));
            PO_HIPCHK(hipMemsetAsync(qst[k].p, 0, sizeof(int32_t) * 2 * (size_t)n, stream));
            if (plan.total_b[k] > 0) wqb = std::max(wqb, po_qual_workspace_bytes(n, in.rows[s], in.max_rows[s], plan.total_b[k], fq.band_size, in.model));
            if (plan.total_u[k] > 0) wqb = std::max(wqb, po_qual_workspace_bytes(n, in.rows[s], in.max_rows[s], plan.total_u[k], 0, in.model));
        }
        PO_HIPCHK(wsq.up(nullptr, wqb));
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {
            const int s = po_pq_side(k);
            const int64_t tb = plan.total_b[k], tu = plan.total_u[k];
            for (int u = 0; u < 2; ++u) {   // the banded call, then the one without a band, each with its own dense layout
                const int64_t tot = u ? tu : tb, at = u ? tb : 0;
                if (tot == 0) continue;
                const int64_t* lo = u ? lou[k].as<int64_t>() : lob[k].as<int64_t>();
                char* lab = labels[k].as<char>() + at;
                double* od = odds[k].as<double>() + at * 5;
                int32_t* q = qst[k].as<int32_t>() + (u ? n : 0);
                po_launch_fastq_gather(scored(in, k), scored(in, k), scored_off(in, k), nullptr, 1, lo, n, tot, lab, stream);
                PO_HIPCHK(hipGetLastError());
                const int rc = po_qual_batch_route(in.y[s], in.y_off[s], n, NOUT, "ACGT", in.model, lab, lo,
                                                   u ? nullptr : guide[k].as<int32_t>(), u ? 0 : fq.band_size, od, logp, q, wsq, wqb, stream,
                                                   qual_route);
                if (rc != PO_OK) return rc;
                if (k < 2) {
                    po_launch_fastq_phred(od, lab, lo, q, off1d[s], n, tot, "ACGT", qual1d, stream);
                    PO_HIPCHK(hipGetLastError());
                }
            }
        }
        po_launch_fastq_pair_phred(odds[2], pos[0], sel[0], qst[2], odds[3], pos[1], sel[1], qst[3], in.seq, in.seq_off, coff, n,
                                   plan.cons_off[n], "ACGT", qual, stream);
        PO_HIPCHK(hipGetLastError());
        return PO_OK;
    }

    // after the synchronise: the characters, the statuses and (where asked for) the odds and the guides.  dev: fq's
    // pointers are device buffers of the caller's (po_pair_qual), filled on `stream`; otherwise host buffers
    int down(const PairQualIn& in, const PairFastqOut& fq, bool dev = false, hipStream_t stream = nullptr) {
        const int n = in.n;
        PO_HIPCHK(po_out(fq.qual1d_h, qual1d.p, s1b, dev, stream));
        PO_HIPCHK(po_out(fq.qual_h, qual.p, cap, dev, stream));
        std::vector<int32_t> st(2 * (size_t)n), qs_dev;
        std::vector<double> dense;
        if (dev) qs_dev.resize(PO_PQ_ITEMS * (size_t)n);
        int32_t* qs = dev ? qs_dev.data() : fq.qual_status_h;
        for (int k = 0; k < PO_PQ_ITEMS; ++k) {
            const int s = po_pq_side(k);
            PO_HIPCHK(qst[k].down(st.data(), sizeof(int32_t) * st.size()));
            for (int i = 0; i < n; ++i) qs[PO_PQ_ITEMS * (size_t)i + k] = po_pair_fastq_status(plan, k, i, st.data());
            double* dst = k < 2 ? fq.odds1d_h : fq.odds_cons_h ? fq.odds_cons_h + (size_t)(k - 2) * 5 * cap : nullptr;
            if (dst && plan.total(k) > 0 && dev) {   // (an optional output: one small copy per item, device to device)
                for (int i = 0; i < n; ++i) {
                    const int64_t L = plan.len[k][i], at = k < 2 ? plan.off1d[s][i] : in.seq_off_h[i];
                    if (L > 0) PO_HIPCHK(po_out(dst + at * 5, odds[k].as<double>() + plan.pos[k][i] * 5, sizeof(double) * 5 * (size_t)L, true, stream));
                }
            } else if (dst && plan.total(k) > 0) {   // dense on the device, at the strings' offsets in the caller's tables
                dense.resize((size_t)plan.total(k) * 5);
                PO_HIPCHK(odds[k].down(dense.data(), sizeof(double) * dense.size()));
                for (int i = 0; i < n; ++i) {
                    const int64_t L = plan.len[k][i], at = k < 2 ? plan.off1d[s][i] : in.seq_off_h[i];
                    if (L > 0) std::memcpy(dst + at * 5, dense.data() + plan.pos[k][i] * 5, sizeof(double) * 5 * (size_t)L);
                }
            }
            if (fq.guide_h && banded)
                PO_HIPCHK(po_out(fq.guide_h + po_pair_fastq_guide_base(k, in.rows[0], in.rows[1]), guide[k].p,
                                 sizeof(int32_t) * (size_t)in.rows[s], dev, stream));
        }
        if (dev) PO_HIPCHK(po_out_h(fq.qual_status_h, qs_dev.data(), sizeof(int32_t) * qs_dev.size(), stream));
        return PO_OK;
    }
};

int check_perm(const std::string& me, const int* perm2_h) {
    for (int c = 0; perm2_h && c < NOUT; ++c)
        if (perm2_h[c] < 0 || perm2_h[c] >= NOUT)
            return po_fail(PO_E_ARG, me + "perm2[" + std::to_string(c) + "] is " + std::to_string(perm2_h[c]) + " (0 to 4)");
    return PO_OK;
}

}  // namespace

extern "C" int po_pair_tables_h(const float* logits_h, const int64_t* row_off_h, int n_reads, const int32_t* pair_idx_h, int n_pairs,
                                int reverse2, const int* perm2_h, double* y1_h, double* y2_h) {
    const std::string me = "po_pair_tables_h: ";
    po_set_error("");
    if (!logits_h || !row_off_h || !pair_idx_h || !y1_h || !y2_h)
        return po_fail(PO_E_ARG, me + "null argument " +
                       (!logits_h ? "logits_h" : !row_off_h ? "row_off_h" : !pair_idx_h ? "pair_idx_h" : !y1_h ? "y1_h" : "y2_h"));
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if (row_off_h[0] != 0) return po_fail(PO_E_ARG, me + "row_off[0] is " + std::to_string(row_off_h[0]) + " (must be 0)");
    for (int r = 0; r < n_reads; ++r)
        if (row_off_h[r + 1] < row_off_h[r]) return po_fail(PO_E_ARG, me + "row_off decreases at read " + std::to_string(r));
    PoPairBasecallPlan pp;
    std::string err;
    int rc = po_pair_basecall_make_plan(row_off_h, n_reads, pair_idx_h, n_pairs, nullptr, nullptr, &pp, &err, "po_pair_tables_h");
    if (rc != PO_OK) return po_fail(rc, err);
    rc = check_perm(me, perm2_h);
    if (rc != PO_OK) return rc;
    if (n_pairs == 0) return PO_OK;
    PoDev lg, so;
    PairTables t;
    PO_HIPCHK(lg.up(logits_h, sizeof(float) * NOUT * (size_t)row_off_h[n_reads]));
    PO_HIPCHK(so.up(row_off_h, sizeof(int64_t) * ((size_t)n_reads + 1)));
    rc = t.up(pp, pair_idx_h, n_pairs);
    if (rc != PO_OK) return rc;
    rc = t.launch(pp, lg, so, n_pairs, reverse2, perm2_h, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(t.y[0].down(y1_h, sizeof(double) * NOUT * (size_t)pp.rows[0]));
    PO_HIPCHK(t.y[1].down(y2_h, sizeof(double) * NOUT * (size_t)pp.rows[1]));
    return PO_OK;
}

// everything a call keeps on the device: one call's, or a po_pair_basecaller worker's between groups and runs
struct PoPairBasecallResident {
    PoBasecallPasses net;
    PairTables t;
    PoSeqOut out;
    PoDev s1o, s1, l1, l2, idn, ws;
    PairFastqStages fs;
};

PoPairBasecallResident* po_pair_basecall_resident_new() { return new PoPairBasecallResident; }
void po_pair_basecall_resident_free(PoPairBasecallResident* st) { delete st; }
PoBasecallPasses& po_pair_basecall_resident_net(PoPairBasecallResident* st) { return st->net; }

// po_pair_basecall_batch_h (fq == NULL), po_pair_basecall_fastq_batch_h and po_pair_basecall_skip_batch_h under their own
// names, and a po_pair_basecaller's groups
int po_pair_basecall_body(PoPairBasecallResident* st, hipStream_t stream, bool signal_resident, const char* name,
                          const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                          const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                          int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                          const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h,
                          double* identity_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                          float* logits_h, float* stage_ms_h, const PoPairBasecallFastq* fq, const int* skip) {
    // skip (or NULL): {skip_threshold, indel_threshold} of --skip_matches: the pair chain is po_skip.hip's plan + run
    const int n_stages = fq ? 8 : 6;
    const std::string me = std::string(name) + ": ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if (n_pairs < 0) return po_fail(PO_E_ARG, me + "n_pairs " + std::to_string(n_pairs));
    const struct { const void* p; const char* name; } ptrs[] = {
        {signal_h, "signal_h"}, {sig_off_h, "sig_off_h"}, {layers_h, "layers_h"}, {weights_h, "weights_h"}, {pair_idx_h, "pair_idx_h"},
        {opt, "opt"}, {seq1d_h, "seq1d_h"}, {seq1d_off_h, "seq1d_off_h"}, {len1_h, "len1_h"}, {len2_h, "len2_h"},
        {identity_h, "identity_h"}, {seq_h, "seq_h"}, {seq_off_h, "seq_off_h"}, {seq_len_h, "seq_len_h"}, {status_h, "status_h"}};
    for (const auto& a : ptrs)
        if (!a.p && !(signal_resident && &a == &ptrs[0])) return po_fail(PO_E_ARG, me + "null argument " + a.name);
    if (fq && null_quality_pointer(me, *fq) != PO_OK) return PO_E_ARG;
    PoBasecallPlan plan;
    PoPairBasecallPlan pp;
    std::string err;
    int rc = po_basecall_make_plan(sig_off_h, n_reads, window, overlap, nullptr, &plan, &err, name);
    if (rc != PO_OK) return po_fail(rc, err);
    rc = po_pair_basecall_make_plan(sig_off_h, n_reads, pair_idx_h, n_pairs, seq1d_off_h, seq_off_h, &pp, &err, name);
    if (rc != PO_OK) return po_fail(rc, err);
    if (reverse_complement != 0 && reverse_complement != 1)
        return po_fail(PO_E_ARG, me + "reverse_complement " + std::to_string(reverse_complement) + " (0 or 1)");
    if (opt->model == PO_MODEL_FLIPFLOP)
        return po_fail(PO_E_UNSUPPORTED, me + "flip-flop decoding (model " + std::to_string(opt->model) +
                       "): the network's output is a CTC table");
    if (opt->model != PO_MODEL_CTC && opt->model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, me + "model " + std::to_string(opt->model));
    if (opt->beam_width < 1 || opt->beam_width > 25)
        return po_fail(PO_E_ARG, me + "beam_width " + std::to_string(opt->beam_width) + " (1 to 25)");
    if (opt->method != PO_METHOD_ROW && opt->method != PO_METHOD_ROW_COL && opt->method != PO_METHOD_GRID)
        return po_fail(PO_E_ARG, me + "method " + std::to_string(opt->method));
    if (skip && (skip[0] < 1 || skip[1] < 1))
        return po_fail(PO_E_ARG, me + "skip_threshold " + std::to_string(skip[0]) + ", indel_threshold " + std::to_string(skip[1]) + " (1 at least)");
    if (skip && opt->diagonal_envelope)
        return po_fail(PO_E_UNSUPPORTED, me + "diagonal_envelope: there is no alignment to take anchors from");
    // the model and the weights' length: po_call_batch's own checks, which come before it looks at a buffer (no windows:
    // the pointers are not followed)
    rc = po_call_batch(weights_h, 0, window, layers_h, n_layers, weights_h, n_weights, (float*)weights_h, nullptr, nullptr, 0,
                       nullptr, nullptr);
    if (rc != PO_OK) return rc;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + n_stages, 0.f);
    if (n_pairs == 0 || n_reads == 0) return PO_OK;

    static const int RC_PERM[NOUT] = {3, 2, 1, 0, 4};   // the complement: A <-> T, C <-> G, blank stays
    PoBasecallPasses& net = st->net;
    PairTables& t = st->t;
    PoSeqOut& out = st->out;
    PoDev &s1o = st->s1o, &s1 = st->s1, &l1 = st->l1, &l2 = st->l2, &idn = st->idn, &ws = st->ws;
    PoDev nab, rws;   // --skip_matches' alone: one-call entries only
    const size_t s1b = (size_t)seq1d_off_h[2 * (size_t)n_pairs], per = sizeof(int32_t) * (size_t)n_pairs;
    rc = net.up(plan, signal_resident ? nullptr : signal_h, sig_off_h, n_reads, window, layers_h, n_layers, weights_h, n_weights, max_windows_per_pass);
    if (rc != PO_OK) return rc;
    rc = t.up(pp, pair_idx_h, n_pairs);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(out.up(seq_off_h, n_pairs));
    PO_HIPCHK(s1o.up(seq1d_off_h, sizeof(int64_t) * (2 * (size_t)n_pairs + 1)));
    PO_HIPCHK(s1.up(nullptr, s1b));
    PO_HIPCHK(l1.up(nullptr, per));
    PO_HIPCHK(l2.up(nullptr, per));
    PO_HIPCHK(idn.up(nullptr, sizeof(double) * (size_t)n_pairs));
    const size_t wsb = skip ? po_skip_plan_ws_bytes(n_pairs, pp.rows[0], pp.rows[1], pp.max_rows[0], pp.max_rows[1], NOUT, opt, skip[0], skip[1])
                            : po_pair_decode_workspace_bytes(n_pairs, pp.rows[0], pp.rows[1], pp.max_rows[0], pp.max_rows[1], NOUT, opt);
    PO_HIPCHK(ws.up(nullptr, wsb));
    if (skip) PO_HIPCHK(nab.up(nullptr, 2 * per));   // anchors and boxes per pair
    PairFastqStages& fs = st->fs;
    PairQualIn qin;
    if (fq) {
        for (int s = 0; s < 2; ++s) { qin.y[s] = t.y[s]; qin.y_off[s] = t.off[s]; qin.rows[s] = pp.rows[s]; qin.max_rows[s] = pp.max_rows[s]; }
        qin.n = n_pairs; qin.model = opt->model;
        qin.seq1d = s1; qin.seq1d_off_h = seq1d_off_h;
        qin.seq = out.seq; qin.seq_off = out.off; qin.seq_off_h = seq_off_h;
        rc = fs.prepare(qin, *fq);
        if (rc != PO_OK) return rc;
    }

    PoSpans stitch(stage_ms_h != nullptr), decode(stage_ms_h != nullptr), guides(stage_ms_h != nullptr), lattice(stage_ms_h != nullptr);
    rc = net.run(plan, window, overlap, layers_h, n_layers, n_weights, stream, stage_ms_h, stitch);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(stitch.mark(stream));
    rc = t.launch(pp, net.logits, net.sig_off, n_pairs, reverse_complement, reverse_complement ? RC_PERM : nullptr, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(stitch.mark(stream));
    PO_HIPCHK(decode.mark(stream));
    if (skip) {   // plan (synchronises: the box totals), the run workspace for those totals, run
        po_skip_totals tot;
        rc = po_launch_skip_plan(t.y[0], t.off[0], t.y[1], t.off[1], n_pairs, NOUT, opt, skip[0], skip[1], pp.rows[0], pp.rows[1],
                                 pp.max_rows[0], pp.max_rows[1], s1, s1o, l1, l2, idn, out.status, nab.as<int32_t>(),
                                 nab.as<int32_t>() + n_pairs, ws, wsb, &tot, stream);
        if (rc != PO_OK) return po_fail(rc, me + "the skip-matches plan was refused");
        const size_t rwsb = po_skip_run_ws_bytes(n_pairs, NOUT, opt, &tot);
        PO_HIPCHK(rws.up(nullptr, rwsb));
        rc = po_launch_skip_run(t.y[0], t.off[0], t.y[1], t.off[1], n_pairs, NOUT, opt, skip[0], skip[1], pp.rows[0], pp.rows[1],
                                pp.max_rows[0], pp.max_rows[1], &tot, ws, wsb, out.seq, out.off, out.len, out.status, rws, rwsb, nullptr,
                                stream);
        if (rc != PO_OK) return po_fail(rc, me + "the skip-matches run was refused");
    } else {
        rc = po_pair_decode_batch(t.y[0], t.off[0], t.y[1], t.off[1], n_pairs, NOUT, opt, s1, s1o, l1, l2, idn, nullptr, out.seq, out.off,
                                  out.len, out.status, ws, wsb, stream);
        if (rc != PO_OK) return rc;
    }
    PO_HIPCHK(decode.mark(stream));
    if (fq) {   // the quality stages, on the tables and the strings the pair chain left on the device
        PO_HIPCHK(guides.mark(stream));
        rc = fs.viterbi(qin, stream);
        if (rc != PO_OK) return rc;
        std::vector<int32_t> h(4 * (size_t)n_pairs);   // statuses | 1-D lengths of side 0 | of side 1 | consensus lengths
        PO_HIPCHK(hipMemcpyAsync(h.data(), out.status.p, per, hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipMemcpyAsync(h.data() + n_pairs, l1.p, per, hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipMemcpyAsync(h.data() + 2 * (size_t)n_pairs, l2.p, per, hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipMemcpyAsync(h.data() + 3 * (size_t)n_pairs, out.len.p, per, hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipStreamSynchronize(stream));
        rc = fs.guides(name, qin, *fq, h.data(), h.data() + n_pairs, h.data() + 2 * (size_t)n_pairs, h.data() + 3 * (size_t)n_pairs, stream);
        if (rc != PO_OK) return rc;
        PO_HIPCHK(guides.mark(stream));
        PO_HIPCHK(lattice.mark(stream));
        rc = fs.lattice(qin, *fq, stream);
        if (rc != PO_OK) return rc;
        PO_HIPCHK(lattice.mark(stream));
    }
    PO_HIPCHK(hipStreamSynchronize(stream));
    if (stage_ms_h) {
        stage_ms_h[4] = stitch.total();
        stage_ms_h[5] = decode.total();
        if (fq) {
            stage_ms_h[6] = guides.total();
            stage_ms_h[7] = lattice.total();
        }
    }
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    PO_HIPCHK(s1.down(seq1d_h, s1b));
    PO_HIPCHK(l1.down(len1_h, per));
    PO_HIPCHK(l2.down(len2_h, per));
    PO_HIPCHK(idn.down(identity_h, sizeof(double) * (size_t)n_pairs));
    PO_HIPCHK(net.logits.down(logits_h, (size_t)plan.rows * NOUT * 4));
    if (fq) {
        rc = fs.down(qin, *fq);
        if (rc != PO_OK) return rc;
    }
    return PO_OK;
}

namespace {
// a call of its own: a fresh state, freed when the call returns, on the null stream
int pair_basecall_impl(const char* name, const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                       const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                       int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                       const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h,
                       double* identity_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                       float* logits_h, float* stage_ms_h, const PairFastqOut* fq, const int* skip = nullptr) {
    PoPairBasecallResident st;
    return po_pair_basecall_body(&st, nullptr, false, name, signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers,
                                 weights_h, n_weights, max_windows_per_pass, pair_idx_h, n_pairs, reverse_complement, opt, seq1d_h,
                                 seq1d_off_h, len1_h, len2_h, identity_h, seq_h, seq_off_h, seq_len_h, status_h, logits_h, stage_ms_h,
                                 fq, skip);
}
}  // namespace

extern "C" int po_pair_basecall_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                        const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                        int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                                        const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                                        int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                                        int32_t* seq_len_h, int32_t* status_h, float* logits_h, float* stage_ms_h) {
    return pair_basecall_impl("po_pair_basecall_batch_h", signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers, weights_h,
                              n_weights, max_windows_per_pass, pair_idx_h, n_pairs, reverse_complement, opt, seq1d_h, seq1d_off_h,
                              len1_h, len2_h, identity_h, seq_h, seq_off_h, seq_len_h, status_h, logits_h, stage_ms_h, nullptr);
}

extern "C" int po_pair_basecall_skip_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                             const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                             int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                                             const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                                             int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                                             int32_t* seq_len_h, int32_t* status_h, float* logits_h, float* stage_ms_h,
                                             int skip_threshold, int indel_threshold) {
    const int skip[2] = {skip_threshold, indel_threshold};
    return pair_basecall_impl("po_pair_basecall_skip_batch_h", signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers,
                              weights_h, n_weights, max_windows_per_pass, pair_idx_h, n_pairs, reverse_complement, opt, seq1d_h,
                              seq1d_off_h, len1_h, len2_h, identity_h, seq_h, seq_off_h, seq_len_h, status_h, logits_h, stage_ms_h, nullptr,
                              skip);
}

extern "C" int po_pair_basecall_fastq_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                              const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                              int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs,
                                              int reverse_complement, const po_pair_options* opt, char* seq1d_h,
                                              const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h, double* identity_h,
                                              char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                                              float* logits_h, int band_size, const int32_t* unbanded_h, char* qual1d_h, char* qual_h,
                                              int32_t* qual_status_h, double* odds1d_h, double* odds_cons_h, int32_t* guide_h,
                                              float* stage_ms_h) {
    const PairFastqOut fq = {band_size, unbanded_h, qual1d_h, qual_h, qual_status_h, odds1d_h, odds_cons_h, guide_h};
    return pair_basecall_impl("po_pair_basecall_fastq_batch_h", signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers,
                              weights_h, n_weights, max_windows_per_pass, pair_idx_h, n_pairs, reverse_complement, opt, seq1d_h,
                              seq1d_off_h, len1_h, len2_h, identity_h, seq_h, seq_off_h, seq_len_h, status_h, logits_h, stage_ms_h, &fq);
}

namespace {

// the refusals that po_pair_qual_h and po_pair_qual share, on host copies of the tables: every table from 0 and
// non-decreasing, a decoded pair's strings within their room
int pair_qual_check(const std::string& me, int n, const int64_t* y1_off_h, const int64_t* y2_off_h, const int64_t* seq1d_off_h,
                    const int64_t* seq_off_h, const int32_t* len1_h, const int32_t* len2_h, const int32_t* seq_len_h,
                    const int32_t* status_h) {
    const struct { const int64_t* off; int count; const char* name; } tables[] = {
        {y1_off_h, n, "y1_off"}, {y2_off_h, n, "y2_off"}, {seq1d_off_h, 2 * n, "seq1d_off"}, {seq_off_h, n, "seq_off"}};
    for (const auto& tb : tables) {
        if (tb.off[0] != 0) return po_fail(PO_E_ARG, me + tb.name + "[0] is " + std::to_string(tb.off[0]) + " (must be 0)");
        for (int i = 0; i < tb.count; ++i)
            if (tb.off[i + 1] < tb.off[i]) return po_fail(PO_E_ARG, me + tb.name + " decreases at item " + std::to_string(i));
    }
    for (int i = 0; i < n; ++i) {
        if (status_h[i] != 0) continue;   // (what a pair that is not decoded holds is not read)
        const int64_t room[3] = {seq1d_off_h[2 * (size_t)i + 1] - seq1d_off_h[2 * (size_t)i],
                                 seq1d_off_h[2 * (size_t)i + 2] - seq1d_off_h[2 * (size_t)i + 1], seq_off_h[i + 1] - seq_off_h[i]};
        const int32_t len[3] = {len1_h[i], len2_h[i], seq_len_h[i]};
        for (int k = 0; k < 3; ++k)
            if (len[k] < 0 || len[k] > room[k])
                return po_fail(PO_E_CAP, me + "pair " + std::to_string(i) + ": " + (k == 0 ? "seq1" : k == 1 ? "seq2" : "the consensus") +
                               " has " + std::to_string(len[k]) + " characters in room for " + std::to_string(room[k]));
    }
    return PO_OK;
}

// the stages on tables and strings that are on the device (in.y, in.seq1d, in.seq, in.seq_off), the rest of `in` filled
// here from the host copies of the tables; dev: fq's outputs are device buffers
int pair_qual_body(const char* name, PairQualIn& in, const PairFastqOut& fq, const int64_t* y1_off_h, const int64_t* y2_off_h,
                   const int64_t* seq1d_off_h, const int64_t* seq_off_h, const int32_t* len1_h, const int32_t* len2_h,
                   const int32_t* seq_len_h, const int32_t* status_h, bool dev, hipStream_t stream) {
    const int n = in.n;
    const int64_t* yo_h[2] = {y1_off_h, y2_off_h};
    for (int s = 0; s < 2; ++s) {
        in.rows[s] = yo_h[s][n];
        in.max_rows[s] = 0;
        for (int i = 0; i < n; ++i) in.max_rows[s] = std::max(in.max_rows[s], yo_h[s][i + 1] - yo_h[s][i]);
    }
    in.seq1d_off_h = seq1d_off_h;
    in.seq_off_h = seq_off_h;
    PairFastqStages fs;
    if (dev) fs.qual_route = po_qual_entry_route();
    int rc = fs.prepare(in, fq);
    if (rc == PO_OK) rc = fs.viterbi(in, stream);
    if (rc == PO_OK) rc = fs.guides(name, in, fq, status_h, len1_h, len2_h, seq_len_h, stream);
    if (rc == PO_OK) rc = fs.lattice(in, fq, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipStreamSynchronize(stream));
    rc = fs.down(in, fq, dev, stream);
    if (rc != PO_OK) return rc;
    if (dev) PO_HIPCHK(hipStreamSynchronize(stream));   // (the stages' buffers are this call's: they go when it returns)
    return PO_OK;
}

}  // namespace

extern "C" int po_pair_qual_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h, int n, int model,
                              const char* seq1d_h, const int64_t* seq1d_off_h, const int32_t* len1_h, const int32_t* len2_h,
                              const char* seq_h, const int64_t* seq_off_h, const int32_t* seq_len_h, const int32_t* status_h,
                              int band_size, const int32_t* unbanded_h, char* qual1d_h, char* qual_h, int32_t* qual_status_h,
                              double* odds1d_h, double* odds_cons_h, int32_t* guide_h) {
    const char* name = "po_pair_qual_h";
    const std::string me = std::string(name) + ": ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n < 0) return po_fail(PO_E_ARG, me + "n " + std::to_string(n));
    const struct { const void* p; const char* name; } ptrs[] = {
        {y1_h, "y1_h"}, {y1_off_h, "y1_off_h"}, {y2_h, "y2_h"}, {y2_off_h, "y2_off_h"}, {seq1d_h, "seq1d_h"}, {seq1d_off_h, "seq1d_off_h"},
        {len1_h, "len1_h"}, {len2_h, "len2_h"}, {seq_h, "seq_h"}, {seq_off_h, "seq_off_h"}, {seq_len_h, "seq_len_h"}, {status_h, "status_h"}};
    for (const auto& a : ptrs)
        if (!a.p) return po_fail(PO_E_ARG, me + "null argument " + a.name);
    const PairFastqOut fq = {band_size, unbanded_h, qual1d_h, qual_h, qual_status_h, odds1d_h, odds_cons_h, guide_h};
    if (null_quality_pointer(me, fq) != PO_OK) return PO_E_ARG;
    if (model == PO_MODEL_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, me + "the flip-flop model has no quality lattice");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, me + "model " + std::to_string(model));
    int rc = pair_qual_check(me, n, y1_off_h, y2_off_h, seq1d_off_h, seq_off_h, len1_h, len2_h, seq_len_h, status_h);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;

    PoDev y[2], yo[2], s1, sq, so;
    PairQualIn in;
    const double* y_h[2] = {y1_h, y2_h};
    const int64_t* yo_h[2] = {y1_off_h, y2_off_h};
    for (int s = 0; s < 2; ++s) {
        PO_HIPCHK(y[s].up(y_h[s], sizeof(double) * NOUT * (size_t)yo_h[s][n]));
        PO_HIPCHK(yo[s].up(yo_h[s], sizeof(int64_t) * ((size_t)n + 1)));
        in.y[s] = y[s]; in.y_off[s] = yo[s];
    }
    PO_HIPCHK(s1.up(seq1d_h, (size_t)seq1d_off_h[2 * (size_t)n]));
    PO_HIPCHK(sq.up(seq_h, (size_t)seq_off_h[n]));
    PO_HIPCHK(so.up(seq_off_h, sizeof(int64_t) * ((size_t)n + 1)));
    in.n = n; in.model = model;
    in.seq1d = s1; in.seq = sq; in.seq_off = so;
    return pair_qual_body(name, in, fq, y1_off_h, y2_off_h, seq1d_off_h, seq_off_h, len1_h, len2_h, seq_len_h, status_h, false, nullptr);
}

// po_pair_qual_h on buffers that are on the device already: the same stages, nothing uploaded but the
// plan's small tables.  The offset tables, lengths and statuses are read back: the plan is made on the host.
extern "C" int po_pair_qual(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int model,
                            const char* seq1d, const int64_t* seq1d_off, const int32_t* len1, const int32_t* len2, const char* seq,
                            const int64_t* seq_off, const int32_t* seq_len, const int32_t* status, int band_size,
                            const int32_t* unbanded_h, char* qual1d, char* qual, int32_t* qual_status, double* odds1d,
                            double* odds_cons, int32_t* guide, void* stream_) {
    const char* name = "po_pair_qual";
    const std::string me = std::string(name) + ": ";
    hipStream_t stream = (hipStream_t)stream_;
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n < 0) return po_fail(PO_E_ARG, me + "n " + std::to_string(n));
    const struct { const void* p; const char* name; } ptrs[] = {
        {y1, "y1"}, {y1_off, "y1_off"}, {y2, "y2"}, {y2_off, "y2_off"}, {seq1d, "seq1d"}, {seq1d_off, "seq1d_off"},
        {len1, "len1"}, {len2, "len2"}, {seq, "seq"}, {seq_off, "seq_off"}, {seq_len, "seq_len"}, {status, "status"},
        {qual1d, "qual1d"}, {qual, "qual"}, {qual_status, "qual_status"}};
    for (const auto& a : ptrs)
        if (!a.p) return po_fail(PO_E_ARG, me + "null argument " + a.name);
    if (model == PO_MODEL_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, me + "the flip-flop model has no quality lattice");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, me + "model " + std::to_string(model));
    if (n == 0) return PO_OK;
    const size_t N = (size_t)n;
    std::vector<int64_t> off(5 * N + 4);   // y1_off | y2_off | seq_off | seq1d_off
    std::vector<int32_t> w(4 * N);         // len1 | len2 | seq_len | status
    int64_t *y1o = off.data(), *y2o = y1o + N + 1, *so = y2o + N + 1, *s1o = so + N + 1;
    PO_HIPCHK(hipMemcpyAsync(y1o, y1_off, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, stream));
    PO_HIPCHK(hipMemcpyAsync(y2o, y2_off, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, stream));
    PO_HIPCHK(hipMemcpyAsync(so, seq_off, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, stream));
    PO_HIPCHK(hipMemcpyAsync(s1o, seq1d_off, sizeof(int64_t) * (2 * N + 1), hipMemcpyDeviceToHost, stream));
    const int32_t* words[4] = {len1, len2, seq_len, status};
    for (int k = 0; k < 4; ++k) PO_HIPCHK(hipMemcpyAsync(w.data() + k * N, words[k], sizeof(int32_t) * N, hipMemcpyDeviceToHost, stream));
    PO_HIPCHK(hipStreamSynchronize(stream));
    const int rc = pair_qual_check(me, n, y1o, y2o, s1o, so, w.data(), w.data() + N, w.data() + 2 * N, w.data() + 3 * N);
    if (rc != PO_OK) return rc;
    const PairFastqOut fq = {band_size, unbanded_h, qual1d, qual, qual_status, odds1d, odds_cons, guide};
    PairQualIn in;
    in.y[0] = y1; in.y_off[0] = y1_off; in.y[1] = y2; in.y_off[1] = y2_off;
    in.n = n; in.model = model;
    in.seq1d = seq1d; in.seq = seq; in.seq_off = seq_off;
    return pair_qual_body(name, in, fq, y1o, y2o, s1o, so, w.data(), w.data() + N, w.data() + 2 * N, w.data() + 3 * N, true, stream);
}
