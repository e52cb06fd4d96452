// The host side of the host-buffer entry points (the *_h twins), once: the thread's error message, a device buffer that frees
// itself, the rebasing of a ragged offset table that need not start at 0, and the read-back of device offset tables.  Host
// only, hidden: nothing here is part of the library's symbol table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#ifndef PO_HOSTBUF_PURE
#include "po_host.h"
#include "po_internal.h"
#endif

#pragma GCC visibility push(hidden)

// ---- ragged tables.  No HIP in this part: tools/hostbuf_check.cpp compiles it alone (PO_HOSTBUF_PURE) under sanitizers.
// A twin's input table off[0..n] may start anywhere (the caller passes a slice of a larger batch): the device gets the items'
// data from element off[0] on and the table minus off[0].
struct PoRagged {
    std::vector<int64_t> off;   // off_h[i] - off_h[0]
    int64_t base = 0;           // off_h[0]: the items' data starts at this element of the caller's array
    int64_t total = 0;          // off_h[n] - off_h[0]
    int64_t max = 0;            // the largest item
    bool ordered = true;        // false only where the check was asked for and the table decreases somewhere
    PoRagged(const int64_t* off_h, int n, bool check_order = false) : off(off_h, off_h + n + 1), base(off_h[0]) {
        for (auto& o : off) o -= base;
        total = off[n];
        for (int i = 0; i < n; ++i) {
            if (check_order && off[i + 1] < off[i]) ordered = false;
            max = std::max(max, off[i + 1] - off[i]);
        }
    }
    size_t bytes() const { return off.size() * sizeof(int64_t); }
};

#ifndef PO_HOSTBUF_PURE
// ---- errors: one thread-local message (po_capi.hip's, the one po_last_error returns)
int po_fail(int code, const std::string& msg);          // sets the message, returns code
int po_fail_hip(hipError_t e, const char* what);        // "what: <HIP's error string>", returns PO_E_HIP
#define PO_HIPCHK(x)                                      \
    do {                                                  \
        hipError_t e_ = (x);                              \
        if (e_ != hipSuccess) return po_fail_hip(e_, #x); \
    } while (0)

// ---- a device buffer that frees itself.  It lives for one call, or, in an engine's resident state, for many: up() keeps
// an allocation that is large enough (grow-only; its contents stay where no source is given), so a later call allocates
// only what has grown.
struct PoDev {
    void* p = nullptr;
    size_t cap = 0;     // bytes allocated
    PoDev() = default;
    PoDev(const PoDev&) = delete;
    PoDev& operator=(const PoDev&) = delete;
    ~PoDev() { if (p) (void)hipFree(p); }
    // allocates `bytes` (256 at least, so that an empty array still has an address) and copies src_h up if there is one
    hipError_t up(const void* src_h, size_t bytes) {
        const size_t need = std::max<size_t>(bytes, 256);
        if (!p || cap < need) {
            if (p) (void)hipFree(p);
            p = nullptr;
            cap = 0;
            hipError_t e = hipMalloc(&p, need);
            if (e != hipSuccess) { p = nullptr; return e; }
            cap = need;
        }
        return src_h && bytes ? hipMemcpy(p, src_h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    }
    hipError_t down(void* dst_h, size_t bytes) const {
        return dst_h && bytes ? hipMemcpy(dst_h, p, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    }
    template <class T> T* as() const { return (T*)p; }
    template <class T> operator T*() const { return (T*)p; }   // an argument of a launch: no cast at the call site
};

// ---- a result on its way out.  A *_h twin's goes to the host with a blocking copy; an entry whose outputs are the caller's
// device buffers (po_fastq_tables, po_pair_qual) gets it on the call's stream.  src_d: device memory; src_h: host memory
// that may go out of scope when the function returns (the device form waits for the copy).
inline hipError_t po_out(void* dst, const void* src_d, size_t bytes, bool dev, hipStream_t s) {
    if (!dst || !bytes) return hipSuccess;
    return dev ? hipMemcpyAsync(dst, src_d, bytes, hipMemcpyDeviceToDevice, s) : hipMemcpy(dst, src_d, bytes, hipMemcpyDeviceToHost);
}
inline hipError_t po_out_h(void* dst, const void* src_h, size_t bytes, hipStream_t s) {
    if (!dst || !bytes) return hipSuccess;
    hipError_t e = hipMemcpyAsync(dst, src_h, bytes, hipMemcpyHostToDevice, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// one ragged input: the items' rows (`width` bytes each) from row r.base of src_h on, and the rebased table
struct PoRows {
    PoDev data, off;
    hipError_t up(const void* src_h, const PoRagged& r, size_t width) {
        const size_t bytes = (size_t)r.total * width;
        hipError_t e = data.up(src_h && bytes ? (const char*)src_h + (size_t)r.base * width : nullptr, bytes);
        return e == hipSuccess ? off.up(r.off.data(), r.bytes()) : e;
    }
};

// the string outputs of a decode: n strings at seq_off_h (an output table: from 0), their lengths and statuses, and the
// log-probabilities where the decoder has them
struct PoSeqOut {
    PoDev off, seq, len, status, logp;
    int n = 0;
    size_t cap = 0;
    hipError_t up(const int64_t* seq_off_h, int n_, bool with_logp = false) {
        n = n_;
        cap = (size_t)seq_off_h[n];
        hipError_t e = off.up(seq_off_h, sizeof(int64_t) * (n + 1));
        if (e == hipSuccess) e = seq.up(nullptr, cap);
        if (e == hipSuccess) e = len.up(nullptr, sizeof(int32_t) * n);
        if (e == hipSuccess && with_logp) e = logp.up(nullptr, sizeof(double) * n);
        if (e == hipSuccess) e = status.up(nullptr, sizeof(int32_t) * n);
        return e;
    }
    hipError_t down(char* seq_h, int32_t* seq_len_h, int32_t* status_h, double* logp_h = nullptr) const {
        hipError_t e = seq.down(seq_h, cap);
        if (e == hipSuccess) e = len.down(seq_len_h, sizeof(int32_t) * n);
        if (e == hipSuccess && logp.p) e = logp.down(logp_h, sizeof(double) * n);
        if (e == hipSuccess) e = status.down(status_h, sizeof(int32_t) * n);
        return e;
    }
};

// ---- device offset tables read back by the device-pointer entry points (small blocking copies on the call's stream)
// ends = {off[0], off[n]}
inline hipError_t po_read_ends(const int64_t* off, int n, hipStream_t s, int64_t ends[2]) {
    hipError_t e = hipMemcpyAsync(&ends[0], off, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&ends[1], off + n, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}
// h[0..n] = a[0..n], h[n + 1..2n + 1] = b[0..n]
inline hipError_t po_read_tables(const int64_t* a, const int64_t* b, int n, hipStream_t s, int64_t* h) {
    hipError_t e = hipMemcpyAsync(h, a, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h + n + 1, b, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}
#endif  // PO_HOSTBUF_PURE

#pragma GCC visibility pop
