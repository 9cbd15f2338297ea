// Tianchi batches built from device-resident recordings (cfg.DATA.device_resident): crop one annotated beat, extend its eight stored leads
// by the four derived limb leads, min-max normalise over all 12 leads and pad / crop to 512 samples.  Definition: include/nefnet_hip.h
// (nef_beat_batch_args); the host path whose bits this reproduces: dataset/tianchi.py, EcgTianChiInterval.__getitem__.
//
// One 256-thread workgroup per sample, two passes over the beat.  Pass 1: lo / hi over 12 leads x n positions in fp64 -- work items are
// (lead unit, group of 8 positions); unit 0 reads leads I and II and also forms the four derived leads, units 1..6 read one stored lead each.
// Pass 2 (the beat is in L2 now): a wave owns one output row at a time, a lane 8 positions = two 16-byte stores.  Both passes read a row
// through load8: the widest loads the address of the row's first element allows, element by element otherwise or where the group crosses
// the beat's end; either way the eight values are the stored ones converted to fp64, so nothing depends on the load form.
// load8, the derived leads, the plan-row check and pass 1 itself live in beat_io.h, shared with recording.hip (nef_beat_range repeats pass 1).
#include "nef_common.h"
#include "beat_io.h"

namespace {

constexpr int BL = NEF_BEAT_LEN;
static_assert(BL == 64 * 8, "a wave writes one output row: 8 positions per lane");

template <typename T>
__global__ __launch_bounds__(256) void beat_batch_kernel(const nef_beat_batch_args a) {
    __shared__ double red[8];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = a.V + 1 + a.R, W = 3 + rows;
    const int64_t* __restrict__ pl = a.plan + (int64_t)b * W;
    const int64_t off = pl[0], stride = pl[1], n64 = pl[2];

    // the plan row is device data the entry point cannot have seen: a row that leaves `signal` reads nothing (block-uniform)
    const bool ok = beat_row_ok(pl, rows, a.signal_elems);

    float* out_row = nullptr;           // pass 2: this wave's row; 8 positions per lane
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.signal);
    if (!ok) {
        const float q = __builtin_nanf("");
        for (int r = wave; r < rows; r += 4) {
            out_row = r < a.V ? a.data + ((int64_t)b * a.V + r) * BL : r == a.V ? a.target_view + (int64_t)b * BL
                                                                                 : a.rest_view + ((int64_t)b * a.R + (r - a.V - 1)) * BL;
            reinterpret_cast<f32x4*>(out_row + 8 * lane)[0] = f32x4{q, q, q, q};
            reinterpret_cast<f32x4*>(out_row + 8 * lane)[1] = f32x4{q, q, q, q};
        }
        return;
    }
    const int n = (int)n64;

    // ---- pass 1: lo, hi
    double lo, hi;
    beat_lo_hi(sig, off, stride, n, red, lo, hi);
    const double span = hi - lo;

    // ---- pass 2: the plan's rows, t < 512
    const int t0 = 8 * lane;
    const int nv = n - t0 < 8 ? (n - t0 < 0 ? 0 : n - t0) : 8;
    for (int r = wave; r < rows; r += 4) {
        const int lead = (int)pl[3 + r];
        out_row = r < a.V ? a.data + ((int64_t)b * a.V + r) * BL : r == a.V ? a.target_view + (int64_t)b * BL
                                                                             : a.rest_view + ((int64_t)b * a.R + (r - a.V - 1)) * BL;
        double s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = 0.0;
        if (nv > 0) {
            if (lead < 8) {
                const int64_t e = off + (int64_t)lead * stride;
                load8(sig + e + t0, nv, elem_align<T>(e), s);
            } else {
                double x[8], y[8];
                load8(sig + off + t0, nv, elem_align<T>(off), x);
                load8(sig + off + stride + t0, nv, elem_align<T>(off + stride), y);
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] = derived(lead - 8, x[i], y[i]);
            }
        }
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = i < nv ? (float)((s[i] - lo) / span) : 0.0f;
        reinterpret_cast<f32x4*>(out_row + t0)[0] = f32x4{v[0], v[1], v[2], v[3]};
        reinterpret_cast<f32x4*>(out_row + t0)[1] = f32x4{v[4], v[5], v[6], v[7]};
    }
}

}  // namespace

extern "C" {

size_t nef_beat_batch_args_bytes(void) { return sizeof(nef_beat_batch_args); }

int nef_beat_batch(const nef_beat_batch_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->signal && a->plan && a->data && a->target_view, NEF_E_NULL);
    NEF_REQUIRE(a->R == 0 || a->rest_view, NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->V >= 1 && a->V <= 12 && a->R >= 0 && a->R <= 64, NEF_E_SHAPE);
    NEF_REQUIRE((a->dtype == 0 || a->dtype == 1) && a->signal_elems >= 1 && a->signal_elems < (1ll << 56), NEF_E_SHAPE);
    const uintptr_t bits = (uintptr_t)a->signal | (uintptr_t)a->data | (uintptr_t)a->target_view | (uintptr_t)a->rest_view;
    NEF_REQUIRE((bits & 15) == 0 && ((uintptr_t)a->plan & 7) == 0, NEF_E_UNSUPPORTED);
    if (a->dtype == 0)
        hipLaunchKernelGGL(beat_batch_kernel<int16_t>, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(beat_batch_kernel<float>, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
