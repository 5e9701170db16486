// ptx_tribox.h -- the BLAS builders' triangle record on the device, shared by the refit (ptx_refit.hip)
// and the builder (ptx_build.hip): scene/bvh.py _triangle_bounds and triangle_boxes, one axis at a time.
#pragma once

#include <hip/hip_runtime.h>

namespace ptx {

// One axis of the builder's record from the three vertices' coordinates: centre and half-extent in f64
// from the f32 positions, the half widened by 2^-24 of the magnitudes, both rounded to f32.  Every
// operation is rounded on its own (no fused multiply-add: the expression is the builder's).
__device__ __forceinline__ void tri_axis_record(float a, float b, float c, float &cf, float &hf) {
#pragma clang fp contract(off)
    const double mn = (double)fminf(a, fminf(b, c)), mx = (double)fmaxf(a, fmaxf(b, c));
    const double half = (mx - mn) / 2.0;
    cf = (float)(mn + half);
    const double wide = (fabs(mn) + half) * 0x1p-24;
    hf = (float)(half + wide);
}

// The builder's triangle bounds: the record's f64 difference and sum rounded to f32; `cf` the centre.
__device__ __forceinline__ void tri_axis_bounds(float a, float b, float c, float &lo, float &hi, float &cf) {
#pragma clang fp contract(off)
    float hf;
    tri_axis_record(a, b, c, cf, hf);
    lo = (float)((double)cf - (double)hf);
    hi = (float)((double)cf + (double)hf);
}
__device__ __forceinline__ void tri_axis_bounds(float a, float b, float c, float &lo, float &hi) {
    float cf;
    tri_axis_bounds(a, b, c, lo, hi, cf);
}

}  // namespace ptx
