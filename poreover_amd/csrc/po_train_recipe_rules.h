// The rules of `train`'s recipe, once: how the global norm of the accumulated gradient is cut into chunks,
// the clip rule, Adam's bias-corrected rate and the decoupled decay, and the update of one element.  po_train.hip's kernels
// and its host code use the same functions.  No HIP in this file: tools/train_recipe_check.cpp compiles it alone under
// sanitizers.
//   norm     sqrt(sum of g[e]²) in f64 (the square of an f32 is exact in f64).  Workgroup b of PO_RECIPE_NORM_WG lanes owns
//            the chunk [b·CHUNK, min((b + 1)·CHUNK, n)); lane l adds, in this order, the squares of elements
//            4·(j·WG + l) + 0..3 of the chunk for j = 0 .. PO_RECIPE_NORM_VECS - 1; a wave adds its lanes by the tree
//            x += x[lane + 32], + 16, .. + 1; the workgroup adds its waves' sums in wave order, one workgroup adds the chunks'
//            sums in chunk order.  The partition is a function of n alone, so the norm is the same bits on every run.
//   clip     tf.clip_by_global_norm: scale = clip_norm / norm where clip_norm > 0 and norm > clip_norm, else 1; the division
//            in f64, rounded to f32 once.  A norm that is not finite marks the record: the update then changes nothing.
//   AdamW    ge = g·scale; m and v as Keras Adam (adam_kernel); p = p − lr_t·m / (sqrt(v) + eps) − (lr·weight_decay)·p: the
//            decay is decoupled and takes the scheduled rate lr, not the bias-corrected lr_t.  With scale = 1 and no decay
//            the element is adam_kernel's bits.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define PO_RC_HD __host__ __device__
#else
#define PO_RC_HD
#endif

constexpr int PO_RECIPE_NORM_WG = 1024;     // lanes of a norm workgroup: 16 waves
constexpr int PO_RECIPE_NORM_VECS = 4;      // 16-byte groups per lane
constexpr int PO_RECIPE_NORM_CHUNK = PO_RECIPE_NORM_WG * PO_RECIPE_NORM_VECS * 4;   // 16 384 floats per workgroup

// what the norm stage leaves on the device for the update, and the host reads with the call's results
struct po_recipe_record {
    double norm;     // of the accumulated gradient, before clipping
    float scale;     // what clipping multiplies the gradient by (1: none)
    int finite;      // 0: the norm is NaN or infinite, the update is skipped
};

// chunks of an n-element gradient (0 for n = 0)
inline int64_t po_recipe_norm_chunks(int64_t n) { return (n + PO_RECIPE_NORM_CHUNK - 1) / PO_RECIPE_NORM_CHUNK; }

// the first element of the j-th 16-byte group of lane l in chunk b
PO_RC_HD inline int64_t po_recipe_norm_elem(int64_t b, int j, int l) {
    return b * PO_RECIPE_NORM_CHUNK + 4 * ((int64_t)j * PO_RECIPE_NORM_WG + l);
}

PO_RC_HD inline float po_recipe_clip_scale(double norm, float clip_norm) {
    return clip_norm > 0.f && norm > (double)clip_norm ? (float)((double)clip_norm / norm) : 1.0f;
}

PO_RC_HD inline po_recipe_record po_recipe_make_record(double sqsum, float clip_norm) {
    po_recipe_record r;
    r.norm = sqrt(sqsum);
    r.scale = po_recipe_clip_scale(r.norm, clip_norm);
    r.finite = r.norm - r.norm == 0.0 ? 1 : 0;     // (NaN and ±inf fail this, every finite value passes)
    return r;
}

// Adam's rate at step t (counted from 1), as po_train_step computes it
inline float po_recipe_lr_t(float lr, float beta1, float beta2, int64_t t) {
    const double td = (double)t;
    return (float)(lr * std::sqrt(1.0 - std::pow((double)beta2, td)) / (1.0 - std::pow((double)beta1, td)));
}

// the factor of the decoupled decay
inline float po_recipe_decay(float lr, float weight_decay) { return lr * weight_decay; }

// one element's update; `decay` 0 adds no term at all
PO_RC_HD inline void po_recipe_adamw(float& p, float& m, float& v, float g, float scale, float lr_t, float b1, float b2,
                                     float eps, float decay) {
    const float ge = g * scale;
    const float me = m + (ge - m) * (1.f - b1);
    const float ve = v + (ge * ge - v) * (1.f - b2);
    m = me;
    v = ve;
    float pn = p - lr_t * me / (sqrtf(ve) + eps);
    if (decay != 0.f) pn = pn - decay * p;
    p = pn;
}
