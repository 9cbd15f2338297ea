// Segment copies / sums of the multi-view train step (SOLVER.train_views; no counterpart in the reference, whose forward takes one
// query angle per step): dst_k[i] = src_k[i] or dst_k[i] += src_k[i] for up to 64 independent segments per launch.  The step uses it
// for the three things that would otherwise be torch kernels inside the replayed graph: the per-view decoder outputs into the loss's
// [3, Q, B, 1, L] layout, the loss gradient back out per view, and the sums over views of the head's gradients.
//
// One writer per element, plain loads and stores, no atomics; the grid is a function of the sizes alone -- the bits are the same
// eagerly, under graph replay and on every rank.  Pointers are slices of larger tensors, so only 4-byte aligned: a segment whose source
// and destination sit at the same offset inside a 16-byte line moves its body as float4 between a scalar head and a scalar tail; any
// other segment is scalar throughout.
#include "nef_common.h"

namespace {

constexpr int COPY_MAX = 64;
struct CopyDesc { const float* src; float* dst; int64_t n; };
struct CopyTable { CopyDesc d[COPY_MAX]; };

template <bool ADD>
__global__ __launch_bounds__(256) void copy_many_kernel(CopyTable t) {
    const CopyDesc& d = t.d[blockIdx.y];
    const float* __restrict__ src = d.src;
    float* __restrict__ dst = d.dst;
    const int64_t n = d.n;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t head = n, n4 = 0;            // scalar elements in front of the 16-byte body, float4s in the body
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {
        head = (int64_t)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
        if (head > n) head = n;
        n4 = (n - head) >> 2;
    }
    for (int64_t i = i0; i < head; i += stride) {
        if (ADD) dst[i] += src[i]; else dst[i] = src[i];
    }
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
    for (int64_t i = i0; i < n4; i += stride) {
        const float4 s = s4[i];
        if (ADD) {
            float4 o = d4[i];
            o.x += s.x, o.y += s.y, o.z += s.z, o.w += s.w;
            d4[i] = o;
        } else {
            d4[i] = s;
        }
    }
    for (int64_t i = head + (n4 << 2) + i0; i < n; i += stride) {
        if (ADD) dst[i] += src[i]; else dst[i] = src[i];
    }
}

}  // namespace

extern "C" int nef_copy_many(const float* const* srcs, float* const* dsts, const int64_t* sizes, int n, int accumulate,
                             nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE((srcs && dsts && sizes) || n <= 0, NEF_E_NULL);
    NEF_REQUIRE(n >= 0 && (accumulate == 0 || accumulate == 1), NEF_E_SHAPE);
    // every check before the first launch: a bad entry behind the 64th segment must not leave half of the segments written
    for (int i = 0; i < n; ++i) {
        NEF_REQUIRE(sizes[i] >= 0, NEF_E_SHAPE);
        NEF_REQUIRE((srcs[i] && dsts[i]) || sizes[i] == 0, NEF_E_NULL);
    }
    if (n == 0) return NEF_OK;
    for (int i0 = 0; i0 < n; i0 += COPY_MAX) {
        CopyTable t;
        const int m = n - i0 < COPY_MAX ? n - i0 : COPY_MAX;
        int64_t biggest = 1;
        for (int i = 0; i < m; ++i) {
            t.d[i] = CopyDesc{srcs[i0 + i], dsts[i0 + i], sizes[i0 + i]};
            if (sizes[i0 + i] > biggest) biggest = sizes[i0 + i];
        }
        // ~4 16-byte transfers per thread on the largest segment.  The latent gradients the step sums over views are hundreds of MB, so
        // the cap is about 8 workgroups per compute unit over the whole launch and not nef_flatten's 128 columns (sized for weight
        // gradients); with many segments the columns shrink so that the short ones do not pay for thousands of idle workgroups
        int gx = (int)nef_cdiv(biggest, 256 * 4 * 4);
        const int cap = 2048 / m > 128 ? 2048 / m : 128;
        if (gx > cap) gx = cap;
        if (gx < 1) gx = 1;
        if (accumulate)
            hipLaunchKernelGGL(copy_many_kernel<true>, dim3((unsigned)gx, (unsigned)m), dim3(256), 0, (hipStream_t)stream, t);
        else
            hipLaunchKernelGGL(copy_many_kernel<false>, dim3((unsigned)gx, (unsigned)m), dim3(256), 0, (hipStream_t)stream, t);
    }
    return nef_launch_status();
}
