// The rules of `train`'s recipe (poreover_amd/csrc/po_train_recipe_rules.h), the part of gradient accumulation, clipping and
// AdamW that needs no device: the same source po_train.hip runs.  Plain C++, no HIP: built and run under
// -fsanitize=address,undefined by tests/test_train_recipe_cpu.py.  Exit status 0 and "ok" when every case holds.
//
// For n = 0 .. 3 chunks + 5 and a few sizes around the weight counts the device tests use: the groups (chunk b, step j, lane l)
// of the norm's partition, cut at n, cover [0, n) exactly once (every element is marked in a heap array of exactly n
// entries), chunk b holds nothing outside [b·CHUNK, (b + 1)·CHUNK), and no chunk is empty.  The sum of squares walked in the
// partition's order (lanes, the wave tree, the waves, the chunks) is held against a plain sum.  The record: the clip rule
// at, below and above the threshold and at clip_norm 0; NaN and both infinities are not finite, the largest double is.  One
// element of AdamW against the expressions of the file's head, and with scale 1 and decay 0 against Keras Adam's.
#include "../poreover_amd/csrc/po_train_recipe_rules.h"

#include <algorithm>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
static long checked = 0;

static void fail(const char* what, long n, long a = 0, long b = 0) {
    if (failures < 20) std::printf("FAILED %s (n %ld: %ld, %ld)\n", what, n, a, b);
    ++failures;
}

static void check_partition(int64_t n) {
    ++checked;
    const int64_t nb = po_recipe_norm_chunks(n);
    if (nb != (n + PO_RECIPE_NORM_CHUNK - 1) / PO_RECIPE_NORM_CHUNK || (n > 0 && nb < 1)) fail("chunk count", n, nb);
    std::vector<unsigned char> seen((size_t)n, 0);
    std::vector<double> g((size_t)n);
    for (int64_t e = 0; e < n; ++e) g[(size_t)e] = (double)((e * 2654435761u) % 1000) / 100.0 - 5.0;
    double total = 0.0, plain = 0.0;
    for (int64_t b = 0; b < nb; ++b) {
        int64_t in_chunk = 0;
        std::vector<double> lane(PO_RECIPE_NORM_WG, 0.0);
        for (int l = 0; l < PO_RECIPE_NORM_WG; ++l)
            for (int j = 0; j < PO_RECIPE_NORM_VECS; ++j) {
                const int64_t e0 = po_recipe_norm_elem(b, j, l);
                for (int k = 0; k < 4; ++k) {
                    const int64_t e = e0 + k;
                    if (e >= n) continue;
                    if (e < b * PO_RECIPE_NORM_CHUNK || e >= (b + 1) * (int64_t)PO_RECIPE_NORM_CHUNK) fail("outside its chunk", n, b, e);
                    ++seen[(size_t)e];
                    ++in_chunk;
                    lane[l] += g[(size_t)e] * g[(size_t)e];
                }
            }
        if (in_chunk == 0) fail("empty chunk", n, b);
        double chunk = 0.0;
        for (int w = 0; w < PO_RECIPE_NORM_WG / 64; ++w) {
            double x[128] = {0.0};
            std::copy(lane.begin() + 64 * w, lane.begin() + 64 * (w + 1), x);
            for (int off = 32; off >= 1; off >>= 1)
                for (int l = 0; l < 64; ++l) x[l] += x[l + off];     // (lanes past the wave add what they hold: lane 0 is right)
            chunk += x[0];
        }
        total += chunk;
    }
    for (int64_t e = 0; e < n; ++e) {
        if (seen[(size_t)e] != 1) { fail("coverage", n, e, seen[(size_t)e]); break; }
        plain += g[(size_t)e] * g[(size_t)e];
    }
    if (std::fabs(total - plain) > 1e-9 * (plain + 1.0)) fail("the sum in partition order", n);
}

int main() {
    static_assert(PO_RECIPE_NORM_CHUNK == 16384, "the device tests name this chunk");
    static_assert(sizeof(po_recipe_record) == 16, "the record is one 16-byte copy");
    const int64_t C = PO_RECIPE_NORM_CHUNK;
    for (int64_t n = 0; n <= 300; ++n) check_partition(n);
    for (int64_t c = 1; c <= 3; ++c)
        for (int64_t d = -5; d <= 5; ++d) check_partition(c * C + d);
    for (int64_t n : {11589, 1000003, 893189}) check_partition(n);

    // the record
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    if (po_recipe_clip_scale(4.0, 0.f) != 1.f || po_recipe_clip_scale(4.0, 4.f) != 1.f || po_recipe_clip_scale(3.0, 4.f) != 1.f)
        fail("a clip that does not bind", 0);
    if (po_recipe_clip_scale(5.0, 1.f) != (float)(1.0 / 5.0) || po_recipe_clip_scale(8.0, 2.f) != 0.25f) fail("a clip that binds", 0);
    po_recipe_record r = po_recipe_make_record(25.0, 1.f);
    if (r.norm != 5.0 || r.scale != 0.2f || r.finite != 1) fail("record of 25", 0);
    r = po_recipe_make_record(0.0, 1.f);
    if (r.norm != 0.0 || r.scale != 1.f || r.finite != 1) fail("record of 0", 0);
    r = po_recipe_make_record(std::numeric_limits<double>::max(), 0.f);
    if (r.finite != 1 || r.scale != 1.f) fail("record of the largest double", 0);
    if (po_recipe_make_record(inf, 1.f).finite != 0 || po_recipe_make_record(nan, 1.f).finite != 0) fail("a non-finite record", 0);
    checked += 9;

    // one element
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-7f, lr = 1e-3f;
    for (int64_t t : {1, 2, 1000}) {
        const float lr_t = po_recipe_lr_t(lr, b1, b2, t);
        const double want = lr * std::sqrt(1.0 - std::pow((double)b2, (double)t)) / (1.0 - std::pow((double)b1, (double)t));
        if (lr_t != (float)want) fail("lr_t", t);
        float p = 0.5f, m = 0.01f, v = 0.0004f;
        po_recipe_adamw(p, m, v, 0.3f, 1.f, lr_t, b1, b2, eps, 0.f);
        const float me = 0.01f + (0.3f - 0.01f) * (1.f - b1), ve = 0.0004f + (0.3f * 0.3f - 0.0004f) * (1.f - b2);
        if (m != me || v != ve || p != 0.5f - lr_t * me / (sqrtf(ve) + eps)) fail("scale 1, no decay: Keras Adam", t);
        float q = 0.5f, mq = 0.01f, vq = 0.0004f;
        const float decay = po_recipe_decay(lr, 0.01f);
        po_recipe_adamw(q, mq, vq, 0.6f, 0.5f, lr_t, b1, b2, eps, decay);
        if (mq != me || vq != ve || q != (0.5f - lr_t * me / (sqrtf(ve) + eps)) - decay * 0.5f) fail("scale and decay", t);
        checked += 3;
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok (%ld cases)\n", checked);
    return 0;
}
