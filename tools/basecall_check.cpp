// The window plan and the argument checks of po_basecall_batch_h (poreover_amd/csrc/po_basecall_plan.h), the part of the
// entry's host side that needs no device.  Plain C++, no HIP: built and run under -fsanitize=address,undefined by
// tests/test_basecall_cpu.py.  Exit status 0 and "ok" when every case holds.
//   - the kept ranges [lo, hi) the stitch kernel uses, against the definition: frame t belongs to window
//     clamp(floor((t - O/2) / S), 0, n - 1) — for W in {1, 2, 7, 8, 40, 41}, every even O < W, 1 <= L <= 4W + 4;
//   - the plan's tables for a ragged batch, each in a heap block of exactly its size;
//   - every refusal, with its code and the value in its message.
#include "../poreover_amd/csrc/po_basecall_plan.h"

#include <cstdio>
#include <cstring>

static int failures = 0;

static void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
    ++failures;
}

static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static void check_rule(int W, int O, int64_t L) {
    const int S = W - O;
    const int64_t n = po_basecall_windows(L, W, S);
    if (O == 0 && n != (L + W - 1) / W) fail("O = 0 is ceil(L / W)", W, O, (long)L);
    if ((n - 1) * S >= L) fail("the last window starts inside the read", W, O, (long)L);
    std::vector<int> owner((size_t)L, -1);
    for (int64_t j = 0; j < n; ++j) {
        int64_t lo, hi;
        po_basecall_keep(j, n, L, S, O, &lo, &hi);
        if (lo >= hi) fail("no window is redundant", W, O, (long)L);
        if (lo < j * S || hi > j * S + W || hi > L) fail("kept frames lie inside their window and the read", W, O, (long)L);
        for (int64_t t = lo; t < hi && t < L; ++t) {
            if (owner[(size_t)t] != -1) fail("one writer per frame", W, O, (long)L);
            owner[(size_t)t] = (int)j;
        }
    }
    for (int64_t t = 0; t < L; ++t) {
        int64_t j = floor_div(t - O / 2, S);
        j = j < 0 ? 0 : j > n - 1 ? n - 1 : j;
        if (owner[(size_t)t] != j) fail("kept range equals the definition", W, O, (long)L);
    }
}

static int plan_of(const std::vector<int64_t>& sig_off, int window, int overlap, const std::vector<int64_t>* seq_off,
                   PoBasecallPlan* p, std::string* err) {
    std::vector<int64_t> a(sig_off);   // exact heap blocks: a read past the table's end is a sanitizer report
    std::vector<int64_t> b(seq_off ? *seq_off : std::vector<int64_t>());
    return po_basecall_make_plan(a.data(), (int)a.size() - 1, window, overlap, seq_off ? b.data() : nullptr, p, err);
}

static void refused(const char* name, const std::vector<int64_t>& sig_off, int window, int overlap,
                    const std::vector<int64_t>* seq_off, int code, const char* needle) {
    PoBasecallPlan p;
    std::string err;
    const int rc = plan_of(sig_off, window, overlap, seq_off, &p, &err);
    if (rc != code || err.find(needle) == std::string::npos) {
        std::printf("FAILED refusal %s: code %d, message \"%s\"\n", name, rc, err.c_str());
        ++failures;
    }
}

int main() {
    const int Ws[] = {1, 2, 7, 8, 40, 41};
    for (int W : Ws)
        for (int O = 0; O < W; O += 2)
            for (int64_t L = 1; L <= 4 * W + 4; ++L) check_rule(W, O, L);

    {   // reads of 1, 40, 41 and 333 samples at W = 40, O = 38 (S = 2): 1, 1, 2 and 148 windows
        PoBasecallPlan p;
        std::string err;
        const std::vector<int64_t> off = {0, 1, 41, 82, 415};
        if (plan_of(off, 40, 38, &off, &p, &err) != PO_OK) fail("ragged plan accepted");
        const std::vector<int64_t> want = {0, 1, 2, 4, 152};
        if (p.win_off != want || p.windows != 152 || p.rows != 415 || p.max_rows != 333 || p.stride != 2) fail("ragged plan tables");
        if (p.win_read.size() != 152 || p.win_read[0] != 0 || p.win_read[1] != 1 || p.win_read[2] != 2 || p.win_read[3] != 2 ||
            p.win_read[4] != 3 || p.win_read[151] != 3)
            fail("ragged plan window -> read");
    }
    {   // no reads
        PoBasecallPlan p;
        std::string err;
        if (plan_of({0}, 40, 8, nullptr, &p, &err) != PO_OK || p.windows != 0 || p.rows != 0 || p.win_off.size() != 1) fail("empty batch");
    }
    const std::vector<int64_t> two = {0, 5, 9}, tight = {0, 5, 8}, zero = {0, 5, 5, 9}, shifted = {3, 8};
    refused("window 0", two, 0, 0, nullptr, PO_E_ARG, "window 0");
    refused("window -3", two, -3, 0, nullptr, PO_E_ARG, "window -3");
    refused("odd overlap", two, 40, 7, nullptr, PO_E_ARG, "overlap 7");
    refused("overlap = window", two, 40, 40, nullptr, PO_E_ARG, "overlap 40");
    refused("overlap > window", two, 40, 42, nullptr, PO_E_ARG, "overlap 42");
    refused("negative overlap", two, 40, -2, nullptr, PO_E_ARG, "overlap -2");
    refused("zero-length read", zero, 40, 8, nullptr, PO_E_ARG, "read 1 has 0 samples");
    refused("decreasing offsets", {0, 5, 3}, 40, 8, nullptr, PO_E_ARG, "read 1 has -2 samples");
    refused("offsets not from 0", shifted, 40, 8, nullptr, PO_E_ARG, "sig_off[0] is 3");
    refused("short sequence capacity", two, 40, 8, &tight, PO_E_CAP, "read 1 has 4 samples and room for 3");
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
