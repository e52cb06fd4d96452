// The quality stages of `basecall --fastq` that run between the decoder and the lattice of po_qual.hip, and after it
// (DESIGN.md §16.5).  The per-element rules are po_fastq_rules.h's; what is here is their launch shape.
//
//   fastq_mode_kernel      one wave per read: is the scored string the Viterbi call (identity), different (to the
//                          aligner), or is there nothing to guide by (diagonal)
//   fastq_gather_kernel    strings at ragged offsets to a dense buffer: the (called, scored) pairs for po_align_batch, the
//                          labels for po_qual_batch; one lane per character
//   fastq_consumed_kernel  one wave per aligned pair, 64 columns a step: a segmented scan by two ballots and two carried
//                          counts, in column order
//   fastq_guide_kernel     one lane per frame: a binary search in the read's frame map
//   fastq_phred_kernel     one lane per base: five float64 log-odds to one character
//
// and of the pair pass, where the scored string, the Viterbi call and the consensus live at offsets of
// their own:
//
//   fastq_mode2_kernel       fastq_mode_kernel with a table for the scored and one for the called string
//   fastq_gather2_kernel     the (called, scored) pairs for po_align_batch, each source at its own table
//   fastq_pair_phred_kernel  one lane per consensus base: the two reads' log-odds, summed where both stand, to one character
//
// No atomics, one writer per value, nothing depends on the launch geometry.
#include <cstring>
#include <string>
#include <vector>

#include "po_fastq_rules.h"
#include "po_hostbuf.h"

namespace {

// the item of a ragged table off[0..n] (off[0] <= k < off[n]) that holds element k; empty items hold none
__device__ __forceinline__ int fq_find(const int64_t* __restrict__ off, int n, int64_t k) {
    int lo = 0, hi = n;   // off[lo] <= k < off[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

unsigned fq_grid(int64_t count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, 256 * 64)); }

}  // namespace

__global__ __launch_bounds__(64) void fastq_mode_kernel(const char* __restrict__ seq, const int32_t* __restrict__ len,
                                                        const char* __restrict__ vseq, const int32_t* __restrict__ vlen,
                                                        const int32_t* __restrict__ vstatus, const int64_t* __restrict__ seq_off,
                                                        int32_t* __restrict__ mode) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int L = len[i], Lc = vlen[i];
    int m = PO_FQ_IDENTITY;
    if (vstatus[i] != PO_OK || L <= 0 || Lc <= 0) m = PO_FQ_DIAGONAL;
    else if (L != Lc) m = PO_FQ_ALIGN;
    else if (seq != vseq) {
        const int64_t o = seq_off[i];
        int differ = 0;
        for (int k = lane; k < L; k += 64) differ |= seq[o + k] != vseq[o + k];
        if (__ballot(differ) != 0ull) m = PO_FQ_ALIGN;
    }
    if (lane == 0) mode[i] = m;
}

// dst[k], dst_off[s] <= k < dst_off[s + 1]: character k - dst_off[s] of string s.  String s is read item[s / per] (item ==
// NULL: s / per itself) of src0 (s % per == 0) or src1 (s % per == 1), at src_off[read].
__global__ __launch_bounds__(256) void fastq_gather_kernel(const char* __restrict__ src0, const char* __restrict__ src1,
                                                           const int64_t* __restrict__ src_off, const int32_t* __restrict__ item,
                                                           int per, const int64_t* __restrict__ dst_off, int n_strings,
                                                           int64_t total, char* __restrict__ dst) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int s = fq_find(dst_off, n_strings, k);
        const int r = item ? item[s / per] : s / per;
        const char* src = (s % per) ? src1 : src0;
        dst[k] = src[src_off[r] + (k - dst_off[s])];
    }
}

struct FqConsumedArgs {
    const char* aln1; const char* aln2; const int64_t* aln_off; const int32_t* ncol; const int32_t* aln_status;
    const int32_t* pair_read;     // the read of pair p, or NULL: p
    const int64_t* out_off;       // consumed of read r at consumed + out_off[r], called_len[r] values
    const int32_t* called_len; const int32_t* label_len;
    int32_t* consumed; int32_t* mode;
};

__global__ __launch_bounds__(64) void fastq_consumed_kernel(FqConsumedArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int r = a.pair_read ? a.pair_read[p] : p;
    const int64_t o = a.aln_off[p];
    const int64_t room = a.aln_off[p + 1] - o;
    int64_t nc = a.ncol[p];
    const bool ok = a.aln_status[p] == PO_OK && nc >= 0 && nc <= room;
    if (!ok) nc = 0;
    const int Lc = a.called_len[r], L = a.label_len[r];
    int32_t* out = a.consumed + a.out_off[r];
    int carry1 = 0, carry2 = 0;
    for (int64_t c0 = 0; c0 < nc; c0 += 64) {
        const int64_t c = c0 + lane;
        const uint64_t m1 = __ballot(c < nc && a.aln1[o + c] != PO_FQ_GAP);
        const uint64_t m2 = __ballot(c < nc && a.aln2[o + c] != PO_FQ_GAP);
        int j;
        int32_t v;
        if (po_fq_consumed_column(m1, m2, lane, carry1, carry2, L, &j, &v) && j < Lc) out[j] = v;
        carry1 += po_fq_popc(m1);
        carry2 += po_fq_popc(m2);
    }
    // (a row 1 that is not the called string, base for base, has no consumed table: the read falls back to the diagonal)
    if (lane == 0) a.mode[r] = (ok && carry1 == Lc) ? PO_FQ_CONSUMED : PO_FQ_DIAGONAL;
}

struct FqGuideArgs {
    const int32_t* map; const int32_t* consumed; const int64_t* y_off; int n; int64_t rows;
    const int32_t* called_len; const int32_t* label_len; const int32_t* mode;
    int32_t* guide;
};

__global__ __launch_bounds__(256) void fastq_guide_kernel(FqGuideArgs a) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.rows; g += (int64_t)gridDim.x * blockDim.x) {
        const int i = fq_find(a.y_off, a.n, g);
        const int64_t r0 = a.y_off[i], T = a.y_off[i + 1] - r0;
        int Lc = a.called_len[i];
        Lc = Lc < 0 ? 0 : (Lc > T ? (int)T : Lc);   // the map has a frame's room per base at most
        a.guide[g] = po_fq_guide(a.map + r0, Lc, a.consumed ? a.consumed + r0 : nullptr, a.mode[i], g - r0, T, a.label_len[i]);
    }
}

struct FqPhredArgs {
    const double* odds; const char* labels; const int64_t* label_off; const int32_t* qstatus; const int64_t* out_off;
    int n; int64_t total; char alphabet[4]; char* qual;
};

__global__ __launch_bounds__(256) void fastq_phred_kernel(FqPhredArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.total; k += (int64_t)gridDim.x * blockDim.x) {
        const int i = fq_find(a.label_off, a.n, k);
        double o[5];
#pragma unroll
        for (int b = 0; b < 5; ++b) o[b] = a.odds[k * 5 + b];
        const int q = a.qstatus[i] != PO_OK ? 0 : po_fq_phred(o, po_fq_code(a.alphabet, a.labels[k]));
        a.qual[a.out_off[i] + (k - a.label_off[i])] = (char)(33 + q);
    }
}

// fastq_mode_kernel for strings that live in two buffers: the scored string of item i at seq + seq_off[i], the Viterbi call
// at vseq + vseq_off[i]
__global__ __launch_bounds__(64) void fastq_mode2_kernel(const char* __restrict__ seq, const int64_t* __restrict__ seq_off,
                                                         const int32_t* __restrict__ len, const char* __restrict__ vseq,
                                                         const int64_t* __restrict__ vseq_off, const int32_t* __restrict__ vlen,
                                                         const int32_t* __restrict__ vstatus, int32_t* __restrict__ mode) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int L = len[i], Lc = vlen[i];
    int m = PO_FQ_IDENTITY;
    if (vstatus[i] != PO_OK || L <= 0 || Lc <= 0) m = PO_FQ_DIAGONAL;
    else if (L != Lc) m = PO_FQ_ALIGN;
    else {
        const int64_t o = seq_off[i], vo = vseq_off[i];
        int differ = 0;
        for (int k = lane; k < L; k += 64) differ |= seq[o + k] != vseq[vo + k];
        if (__ballot(differ) != 0ull) m = PO_FQ_ALIGN;
    }
    if (lane == 0) mode[i] = m;
}

// dst[k], dst_off[s] <= k < dst_off[s + 1], for the `total` characters from dst_off[0] on: character k - dst_off[s] of
// string s, which is the called (s even: src0 at off0[r]) or the scored (s odd: src1 at off1[r]) string of item r = item[s / 2]
__global__ __launch_bounds__(256) void fastq_gather2_kernel(const char* __restrict__ src0, const int64_t* __restrict__ off0,
                                                            const char* __restrict__ src1, const int64_t* __restrict__ off1,
                                                            const int32_t* __restrict__ item, const int64_t* __restrict__ dst_off,
                                                            int n_strings, int64_t base, int64_t total, char* __restrict__ dst) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = base + j;
        const int s = fq_find(dst_off, n_strings, k);
        const int r = item[s / 2];
        const int64_t c = k - dst_off[s];
        dst[k] = (s & 1) ? src1[off1[r] + c] : src0[off0[r] + c];
    }
}

struct FqPairPhredArgs {
    const double* odds1; const double* odds2;     // five float64 per base
    const int64_t* pos1; const int64_t* pos2;     // the first odds row of pair i's consensus on either side
    const int32_t* sel1; const int32_t* sel2;     // the entry of qst1 / qst2 that holds the pair's status, or NULL: i
    const int32_t* qst1; const int32_t* qst2;
    const char* seq; const int64_t* seq_off;      // the consensus strings; the characters go to qual at the same offsets
    const int64_t* dense_off;                     // [n + 1] the consensus lengths, summed: one lane per base
    int n; int64_t total; char alphabet[4]; char* qual;
};

__global__ __launch_bounds__(256) void fastq_pair_phred_kernel(FqPairPhredArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.total; k += (int64_t)gridDim.x * blockDim.x) {
        const int i = fq_find(a.dense_off, a.n, k);
        const int64_t j = k - a.dense_off[i];
        const bool ok1 = a.qst1[a.sel1 ? a.sel1[i] : i] == PO_OK, ok2 = a.qst2[a.sel2 ? a.sel2[i] : i] == PO_OK;
        const double* p1 = a.odds1 + (a.pos1[i] + j) * 5;
        const double* p2 = a.odds2 + (a.pos2[i] + j) * 5;
        double o1[5], o2[5];
#pragma unroll
        for (int b = 0; b < 5; ++b) { o1[b] = p1[b]; o2[b] = p2[b]; }
        const int64_t at = a.seq_off[i] + j;
        a.qual[at] = (char)(33 + po_fq_pair_phred(o1, o2, ok1, ok2, po_fq_code(a.alphabet, a.seq[at])));
    }
}

// ------------------------------------------------------------------------------------------------------------ launches
extern "C" {

int po_launch_fastq_mode(const char* seq, const int32_t* len, const char* vseq, const int32_t* vlen, const int32_t* vstatus,
                         const int64_t* seq_off, int n, int32_t* mode, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    hipLaunchKernelGGL(fastq_mode_kernel, dim3(n), dim3(64), 0, stream, seq, len, vseq, vlen, vstatus, seq_off, mode);
    return PO_OK;
}

int po_launch_fastq_gather(const char* src0, const char* src1, const int64_t* src_off, const int32_t* item, int per,
                           const int64_t* dst_off, int n_strings, int64_t total, char* dst, hipStream_t stream) {
    if (n_strings <= 0 || total <= 0) return PO_OK;
    hipLaunchKernelGGL(fastq_gather_kernel, dim3(fq_grid(total)), dim3(256), 0, stream, src0, src1, src_off, item, per, dst_off,
                       n_strings, total, dst);
    return PO_OK;
}

int po_launch_fastq_consumed(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol,
                             const int32_t* aln_status, int n_pairs, const int32_t* pair_read, const int64_t* out_off,
                             const int32_t* called_len, const int32_t* label_len, int32_t* consumed, int32_t* mode,
                             hipStream_t stream) {
    if (n_pairs <= 0) return PO_OK;
    FqConsumedArgs a = {aln1, aln2, aln_off, ncol, aln_status, pair_read, out_off, called_len, label_len, consumed, mode};
    hipLaunchKernelGGL(fastq_consumed_kernel, dim3(n_pairs), dim3(64), 0, stream, a);
    return PO_OK;
}

int po_launch_fastq_guide(const int32_t* map, const int32_t* consumed, const int64_t* y_off, int n, int64_t rows,
                          const int32_t* called_len, const int32_t* label_len, const int32_t* mode, int32_t* guide,
                          hipStream_t stream) {
    if (n <= 0 || rows <= 0) return PO_OK;
    FqGuideArgs a = {map, consumed, y_off, n, rows, called_len, label_len, mode, guide};
    hipLaunchKernelGGL(fastq_guide_kernel, dim3(fq_grid(rows)), dim3(256), 0, stream, a);
    return PO_OK;
}

int po_launch_fastq_phred(const double* odds, const char* labels, const int64_t* label_off, const int32_t* qstatus,
                          const int64_t* out_off, int n, int64_t total, const char* alphabet, char* qual, hipStream_t stream) {
    if (n <= 0 || total <= 0) return PO_OK;
    FqPhredArgs a = {odds, labels, label_off, qstatus, out_off, n, total, {0, 0, 0, 0}, qual};
    std::memcpy(a.alphabet, alphabet ? alphabet : "ACGT", 4);
    hipLaunchKernelGGL(fastq_phred_kernel, dim3(fq_grid(total)), dim3(256), 0, stream, a);
    return PO_OK;
}

int po_launch_fastq_mode2(const char* seq, const int64_t* seq_off, const int32_t* len, const char* vseq, const int64_t* vseq_off,
                          const int32_t* vlen, const int32_t* vstatus, int n, int32_t* mode, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    hipLaunchKernelGGL(fastq_mode2_kernel, dim3(n), dim3(64), 0, stream, seq, seq_off, len, vseq, vseq_off, vlen, vstatus, mode);
    return PO_OK;
}

int po_launch_fastq_gather2(const char* src0, const int64_t* off0, const char* src1, const int64_t* off1, const int32_t* item,
                            const int64_t* dst_off, int n_strings, int64_t base, int64_t total, char* dst, hipStream_t stream) {
    if (n_strings <= 0 || total <= 0) return PO_OK;
    hipLaunchKernelGGL(fastq_gather2_kernel, dim3(fq_grid(total)), dim3(256), 0, stream, src0, off0, src1, off1, item, dst_off,
                       n_strings, base, total, dst);
    return PO_OK;
}

int po_launch_fastq_pair_phred(const double* odds1, const int64_t* pos1, const int32_t* sel1, const int32_t* qst1,
                               const double* odds2, const int64_t* pos2, const int32_t* sel2, const int32_t* qst2, const char* seq,
                               const int64_t* seq_off, const int64_t* dense_off, int n, int64_t total, const char* alphabet,
                               char* qual, hipStream_t stream) {
    if (n <= 0 || total <= 0) return PO_OK;
    FqPairPhredArgs a = {odds1, odds2, pos1, pos2, sel1, sel2, qst1, qst2, seq, seq_off, dense_off, n, total, {0, 0, 0, 0}, qual};
    std::memcpy(a.alphabet, alphabet ? alphabet : "ACGT", 4);
    hipLaunchKernelGGL(fastq_pair_phred_kernel, dim3(fq_grid(total)), dim3(256), 0, stream, a);
    return PO_OK;
}

// ------------------------------------------------------------------------------------------------------------ host buffers
// The three stages alone, for the tests: tables from 0, non-decreasing.
static int fq_check_table(const char* me, const char* name, const int64_t* off_h, int n) {
    if (off_h[0] != 0) return po_fail(PO_E_ARG, std::string(me) + ": " + name + "[0] is " + std::to_string(off_h[0]) + " (must be 0)");
    for (int i = 0; i < n; ++i)
        if (off_h[i + 1] < off_h[i]) return po_fail(PO_E_ARG, std::string(me) + ": " + name + " decreases at item " + std::to_string(i));
    return PO_OK;
}

int po_fastq_guide_h(const int32_t* map_h, const int32_t* consumed_h, const int64_t* y_off_h, int n, const int32_t* called_len_h,
                     const int32_t* label_len_h, const int32_t* mode_h, int32_t* guide_h) {
    const char* me = "po_fastq_guide_h";
    po_set_error("");
    if (n < 0) return po_fail(PO_E_ARG, std::string(me) + ": n " + std::to_string(n));
    if (n == 0) return PO_OK;
    if (!y_off_h || !called_len_h || !label_len_h || !mode_h) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    int rc = fq_check_table(me, "y_off", y_off_h, n);
    if (rc != PO_OK) return rc;
    const int64_t rows = y_off_h[n];
    if (rows > 0 && (!map_h || !guide_h)) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    for (int i = 0; i < n; ++i) {
        const int64_t T = y_off_h[i + 1] - y_off_h[i];
        if (called_len_h[i] < 0 || called_len_h[i] > T || label_len_h[i] < 0 || mode_h[i] < PO_FQ_IDENTITY || mode_h[i] > PO_FQ_DIAGONAL ||
            (mode_h[i] == PO_FQ_CONSUMED && !consumed_h))
            return po_fail(PO_E_ARG, std::string(me) + ": read " + std::to_string(i) + " has " + std::to_string(called_len_h[i]) +
                           " called bases on " + std::to_string(T) + " frames, " + std::to_string(label_len_h[i]) +
                           " scored bases, mode " + std::to_string(mode_h[i]));
    }
    PoDev mp, cs, yo, cl, ll, md, gd;
    PO_HIPCHK(mp.up(map_h, sizeof(int32_t) * rows));
    if (consumed_h) PO_HIPCHK(cs.up(consumed_h, sizeof(int32_t) * rows));
    PO_HIPCHK(yo.up(y_off_h, sizeof(int64_t) * ((size_t)n + 1)));
    PO_HIPCHK(cl.up(called_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(ll.up(label_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(md.up(mode_h, sizeof(int32_t) * n));
    PO_HIPCHK(gd.up(nullptr, sizeof(int32_t) * rows));
    po_launch_fastq_guide(mp, cs, yo, n, rows, cl, ll, md, gd, nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(gd.down(guide_h, sizeof(int32_t) * rows));
    return PO_OK;
}

int po_fastq_consumed_h(const char* aln1_h, const char* aln2_h, const int64_t* aln_off_h, const int32_t* ncol_h, int n,
                        const int32_t* called_len_h, const int32_t* label_len_h, const int64_t* out_off_h, int32_t* consumed_h,
                        int32_t* mode_h) {
    const char* me = "po_fastq_consumed_h";
    po_set_error("");
    if (n < 0) return po_fail(PO_E_ARG, std::string(me) + ": n " + std::to_string(n));
    if (n == 0) return PO_OK;
    if (!aln_off_h || !ncol_h || !called_len_h || !label_len_h || !out_off_h || !mode_h) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    int rc = fq_check_table(me, "aln_off", aln_off_h, n);
    if (rc == PO_OK) rc = fq_check_table(me, "out_off", out_off_h, n);
    if (rc != PO_OK) return rc;
    if ((aln_off_h[n] > 0 && (!aln1_h || !aln2_h)) || (out_off_h[n] > 0 && !consumed_h)) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    for (int i = 0; i < n; ++i)
        if (ncol_h[i] < 0 || ncol_h[i] > aln_off_h[i + 1] - aln_off_h[i] || called_len_h[i] < 0 ||
            called_len_h[i] > out_off_h[i + 1] - out_off_h[i] || label_len_h[i] < 0)
            return po_fail(PO_E_ARG, std::string(me) + ": pair " + std::to_string(i) + " has " + std::to_string(ncol_h[i]) +
                           " columns in room for " + std::to_string(aln_off_h[i + 1] - aln_off_h[i]) + ", " +
                           std::to_string(called_len_h[i]) + " called bases in room for " +
                           std::to_string(out_off_h[i + 1] - out_off_h[i]) + ", " + std::to_string(label_len_h[i]) + " scored bases");
    PoDev a1, a2, ao, nc, st, cl, ll, oo, cs, md;
    PO_HIPCHK(a1.up(aln1_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(a2.up(aln2_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(ao.up(aln_off_h, sizeof(int64_t) * ((size_t)n + 1)));
    PO_HIPCHK(nc.up(ncol_h, sizeof(int32_t) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(hipMemset(st.p, 0, sizeof(int32_t) * n));
    PO_HIPCHK(cl.up(called_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(ll.up(label_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(oo.up(out_off_h, sizeof(int64_t) * ((size_t)n + 1)));
    PO_HIPCHK(cs.up(nullptr, sizeof(int32_t) * (size_t)out_off_h[n]));
    PO_HIPCHK(hipMemset(cs.p, 0, std::max<size_t>(sizeof(int32_t) * (size_t)out_off_h[n], 256)));
    PO_HIPCHK(md.up(nullptr, sizeof(int32_t) * n));
    po_launch_fastq_consumed(a1, a2, ao, nc, st, n, nullptr, oo, cl, ll, cs, md, nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(cs.down(consumed_h, sizeof(int32_t) * (size_t)out_off_h[n]));
    PO_HIPCHK(md.down(mode_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_fastq_phred_h(const double* odds_h, const char* labels_h, const int64_t* label_off_h, int n, const char* alphabet,
                     const int32_t* qual_status_h, char* qual_h) {
    const char* me = "po_fastq_phred_h";
    po_set_error("");
    if (n < 0) return po_fail(PO_E_ARG, std::string(me) + ": n " + std::to_string(n));
    if (n == 0) return PO_OK;
    if (!label_off_h || !qual_status_h) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    if (alphabet && std::strlen(alphabet) != 4) return po_fail(PO_E_ARG, std::string(me) + ": alphabet \"" + alphabet + "\" (4 symbols)");
    const int rc = fq_check_table(me, "label_off", label_off_h, n);
    if (rc != PO_OK) return rc;
    const int64_t total = label_off_h[n];
    if (total > 0 && (!odds_h || !labels_h || !qual_h)) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    PoDev od, lb, lo, qs, ql;
    PO_HIPCHK(od.up(odds_h, sizeof(double) * 5 * (size_t)total));
    PO_HIPCHK(lb.up(labels_h, (size_t)total));
    PO_HIPCHK(lo.up(label_off_h, sizeof(int64_t) * ((size_t)n + 1)));
    PO_HIPCHK(qs.up(qual_status_h, sizeof(int32_t) * n));
    PO_HIPCHK(ql.up(nullptr, (size_t)total));
    po_launch_fastq_phred(od, lb, lo, qs, lo, n, total, alphabet, ql, nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ql.down(qual_h, (size_t)total));
    return PO_OK;
}

int po_fastq_pair_phred_h(const double* odds1_h, const double* odds2_h, const char* labels_h, const int64_t* label_off_h, int n,
                          const char* alphabet, const int32_t* st1_h, const int32_t* st2_h, char* qual_h) {
    const char* me = "po_fastq_pair_phred_h";
    po_set_error("");
    if (n < 0) return po_fail(PO_E_ARG, std::string(me) + ": n " + std::to_string(n));
    if (n == 0) return PO_OK;
    if (!label_off_h || !st1_h || !st2_h)
        return po_fail(PO_E_ARG, std::string(me) + ": null argument " + (!label_off_h ? "label_off_h" : !st1_h ? "st1_h" : "st2_h"));
    if (alphabet && std::strlen(alphabet) != 4) return po_fail(PO_E_ARG, std::string(me) + ": alphabet \"" + alphabet + "\" (4 symbols)");
    const int rc = fq_check_table(me, "label_off", label_off_h, n);
    if (rc != PO_OK) return rc;
    const int64_t total = label_off_h[n];
    if (total > 0 && (!odds1_h || !odds2_h || !labels_h || !qual_h))
        return po_fail(PO_E_ARG, std::string(me) + ": null argument " +
                       (!odds1_h ? "odds1_h" : !odds2_h ? "odds2_h" : !labels_h ? "labels_h" : "qual_h"));
    PoDev o1, o2, lb, lo, s1, s2, ql;
    PO_HIPCHK(o1.up(odds1_h, sizeof(double) * 5 * (size_t)total));
    PO_HIPCHK(o2.up(odds2_h, sizeof(double) * 5 * (size_t)total));
    PO_HIPCHK(lb.up(labels_h, (size_t)total));
    PO_HIPCHK(lo.up(label_off_h, sizeof(int64_t) * ((size_t)n + 1)));
    PO_HIPCHK(s1.up(st1_h, sizeof(int32_t) * n));
    PO_HIPCHK(s2.up(st2_h, sizeof(int32_t) * n));
    PO_HIPCHK(ql.up(nullptr, (size_t)total));
    po_launch_fastq_pair_phred(o1, lo, nullptr, s1, o2, lo, nullptr, s2, lb, lo, lo, n, total, alphabet, ql, nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ql.down(qual_h, (size_t)total));
    return PO_OK;
}

}  // extern "C"
