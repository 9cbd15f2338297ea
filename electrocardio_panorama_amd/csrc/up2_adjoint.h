// Adjoint of Upsample(x2, linear, align_corners=False), one input position at a time.  One definition for the kernels that rebuild it
// while they read a 2*Tin-long gradient row (elementwise.hip's mix backward, lead_mask.hip): their bits agree with the two-pass form.
#pragma once
#include "nef_common.h"

__device__ __forceinline__ float up2_bwd_edge(const float* __restrict__ gr, int Tin, int m) {
    const int To = 2 * Tin;
    float s = 0.f;
#pragma unroll
    for (int d = -1; d <= 2; ++d) {
        const int i = 2 * m + d;
        if (i < 0 || i >= To) continue;
        float src = 0.5f * ((float)i + 0.5f) - 0.5f;
        if (src < 0.f) src = 0.f;
        int i0 = (int)src;
        if (i0 > Tin - 1) i0 = Tin - 1;
        const int i1 = i0 + (i0 < Tin - 1 ? 1 : 0);
        const float l1 = src - (float)i0;
        const float l0 = 1.f - l1;
        const float g = gr[i];
        if (i0 == m) s += l0 * g;
        if (i1 == m) s += l1 * g;
    }
    return s;
}

// adjoint of Upsample(x2, linear, align_corners=False) at input position m, read from the 2*Tin-long gradient row `gr`
// (the expression of upsample2_bwd_rows, so a consumer that rebuilds it on the fly is bit-identical to the two-pass form)
__device__ __forceinline__ float up2_adjoint(const float* __restrict__ gr, int Tin, int m) {
    if (m == 0 || m == Tin - 1) return up2_bwd_edge(gr, Tin, m);
    return 0.25f * gr[2 * m - 1] + 0.75f * gr[2 * m] + 0.75f * gr[2 * m + 1] + 0.25f * gr[2 * m + 2];
}
