// Whole recordings from per-beat views (recording.py): the inverse direction of nef_beat_batch.  Definitions:
// include/nefnet_hip.h (nef_beat_range_args, nef_beat_stitch_args, nef_recording_stats_args).
//
// nef_beat_range       lo / hi of every plan row -- pass 1 of beat_batch_kernel (beat_io.h) and nothing else; one workgroup per row.
// nef_beat_stitch      de-normalises [Bt, A, 512] views with those ranges and writes them at the beats' P onsets of [A, len] signals: a block
//                      is (beat, four angles), a wave one angle row, a lane 8 positions; the tail of a beat longer than 512 is strided over
//                      the wave.
// nef_recording_stats  per (recording, angle) the count and six fp64 sums of the stitched signal against a stored or derived lead: wave w
//                      takes the recording's beats w, w + 4, ..., lane l of it the groups of 8 positions l, l + 64, ...; shuffle tree, then
//                      the four waves in order -- the assignment and the order depend on the recording's own tables only.
//
// No kernel keeps state, uses an atomic or scratch; every output element has one writer.  views and out may sit at any 4-byte address:
// a row whose first element is 16-byte aligned moves in 16-byte accesses, any other element by element, the values being the same.
#include "nef_common.h"
#include "beat_io.h"

namespace {

constexpr int BL = NEF_BEAT_LEN;
static_assert(BL == 64 * 8, "a wave reads one view row: 8 positions per lane");

// bytes (16, 8 or 4) to which a float's address is aligned
__device__ __forceinline__ int ptr_align(const float* p) {
    const int a = (int)((uintptr_t)p & 15u);
    return a == 0 ? 16 : (a & -a);
}

__device__ __forceinline__ bool finite_d(double x) { return x - x == 0.0; }

// ------------------------------------------------------------------------------------------------------------ nef_beat_range
template <typename T>
__global__ __launch_bounds__(256) void beat_range_kernel(const nef_beat_range_args a) {
    __shared__ double red[8];
    const int b = (int)blockIdx.x, rows = a.V + 1 + a.R;
    const int64_t* __restrict__ pl = a.plan + (int64_t)b * (3 + rows);
    double lo = __builtin_nan(""), hi = lo;
    if (beat_row_ok(pl, rows, a.signal_elems))          // block-uniform
        beat_lo_hi(reinterpret_cast<const T*>(a.signal), pl[0], pl[1], (int)pl[2], red, lo, hi);
    if (threadIdx.x == 0) {
        a.range[2 * (int64_t)b] = lo;
        a.range[2 * (int64_t)b + 1] = hi;
    }
}

// ------------------------------------------------------------------------------------------------------------ nef_beat_stitch
// lo + v * span in fp64 (one multiply, one add); NaN for a range that is not finite
__device__ __forceinline__ double denorm(float v, double lo, double span, bool fin) {
    return fin ? lo + (double)v * span : __builtin_nan("");
}

__global__ __launch_bounds__(256) void beat_stitch_kernel(const nef_beat_stitch_args a) {
    const int b = (int)blockIdx.y, lane = (int)threadIdx.x & 63, ang = 4 * (int)blockIdx.x + ((int)threadIdx.x >> 6);
    const int64_t* __restrict__ row = a.table + 4 * (int64_t)b;
    const int64_t base = row[0], stride = row[1], n64 = row[2];
    // the table is device data: a row that would leave `out` writes nothing (block-uniform; A <= 2^16 and out_elems < 2^40, so no product wraps)
    const bool ok = base >= 0 && base < a.out_elems && stride >= 1 && stride <= a.out_elems && n64 >= 1 && n64 <= stride &&
                    n64 <= 0x7FFF0000ll && base + (int64_t)(a.A - 1) * stride + n64 <= a.out_elems;
    if (!ok || ang >= a.A) return;
    const int n = (int)n64;
    const double lo = a.range[2 * (int64_t)b], hi = a.range[2 * (int64_t)b + 1], span = hi - lo;
    const bool fin = finite_d(span);
    const float* __restrict__ v = a.views + (int64_t)b * a.view_bs + (int64_t)ang * a.view_as;
    float* __restrict__ o = a.out + base + (int64_t)ang * stride;

    const int t0 = 8 * lane, m = n < BL ? n : BL;
    const int nv = m - t0 < 8 ? (m - t0 < 0 ? 0 : m - t0) : 8;
    if (nv > 0) {
        float x[8];
        if (ptr_align(v) == 16) {
            const f32x4 q0 = reinterpret_cast<const f32x4*>(v + t0)[0], q1 = reinterpret_cast<const f32x4*>(v + t0)[1];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = q0[i], x[4 + i] = q1[i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = i < nv ? v[t0 + i] : 0.0f;
        }
        float y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = (float)denorm(x[i], lo, span, fin);
        if (nv == 8 && ptr_align(o) == 16) {
            reinterpret_cast<f32x4*>(o + t0)[0] = f32x4{y[0], y[1], y[2], y[3]};
            reinterpret_cast<f32x4*>(o + t0)[1] = f32x4{y[4], y[5], y[6], y[7]};
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < nv) o[t0 + i] = y[i];
        }
    }
    if (n <= BL) return;

    // ---- the tail of a beat longer than the row: NaN, or the bridge from this beat's last value to the next beat's first (hold without one)
    if (a.fill == 0) {
        const float q = __builtin_nanf("");
        for (int t = BL + lane; t < n; t += 64) o[t] = q;
        return;
    }
    const double a0 = denorm(v[BL - 1], lo, span, fin);
    double a1 = a0;
    if (row[3] == 1 && b + 1 < a.Bt) {
        const double lo1 = a.range[2 * (int64_t)b + 2], span1 = a.range[2 * (int64_t)b + 3] - lo1;
        a1 = denorm(v[a.view_bs], lo1, span1, finite_d(span1));
    }
    const double d = a1 - a0, len = (double)(n - (BL - 1));
    for (int t = BL + lane; t < n; t += 64) o[t] = (float)(a0 + d * ((double)(t - (BL - 1)) / len));
}

// ------------------------------------------------------------------------------------------------------------ nef_recording_stats
template <typename T>
__global__ __launch_bounds__(256) void recording_stats_kernel(const nef_recording_stats_args a) {
    __shared__ double red[4][7];
    __shared__ int bad_any;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rec = (int)(blockIdx.x / (unsigned)a.A), ang = (int)(blockIdx.x % (unsigned)a.A);
    double* __restrict__ res = a.stats + ((int64_t)rec * a.A + ang) * 7;
    const int lead = a.score_leads[ang];
    if (lead == -1) {                                   // block-uniform
        if (tid < 7) res[tid] = 0.0;
        return;
    }
    const int64_t* __restrict__ rr = a.rec_table + 4 * (int64_t)rec;
    const int64_t first = rr[0], nrows = rr[1], soff = rr[2], len = rr[3], ooff = a.out_offsets[rec];
    // the tables are device data: a recording that would leave `signal` or `out`, a beat outside its recording or a lead outside 0..11 reads
    // nothing and gives NaNs (block-uniform)
    bool ok = lead >= 0 && lead < 12 && first >= 0 && nrows >= 0 && nrows <= a.Bt && first <= a.Bt - nrows && soff >= 0 && len >= 1 &&
              len <= 0x7FFF0000ll && len <= a.signal_elems && soff <= a.signal_elems - 8 * len && ooff >= 0 && len <= a.out_elems &&
              ooff <= a.out_elems - (int64_t)a.A * len;
    if (tid == 0) bad_any = 0;
    __syncthreads();
    if (ok) {
        bool bad = false;
        for (int64_t k = tid; k < nrows; k += 256) {
            const int64_t* __restrict__ bt = a.beat_table + 4 * (first + k);
            const int64_t p = bt[0] - ooff;
            bad = bad || p < 0 || bt[1] != len || bt[2] < 1 || bt[2] > len || p > len - bt[2];
        }
        if (bad) bad_any = 1;                           // every writer stores the same word
    }
    __syncthreads();
    if (!ok || bad_any) {
        if (tid < 7) res[tid] = __builtin_nan("");
        return;
    }
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.signal) + soff;
    const float* __restrict__ pred = a.out + ooff + (int64_t)ang * len;

    auto truth8 = [&](int64_t pos, int nv, double (&y)[8]) {
        if (lead < 8) {
            const int64_t e = soff + (int64_t)lead * len + pos;
            load8(sig + (e - soff), nv, elem_align<T>(e), y);
        } else {
            double p[8], q[8];
            load8(sig + pos, nv, elem_align<T>(soff + pos), p);
            load8(sig + len + pos, nv, elem_align<T>(soff + len + pos), q);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = derived(lead - 8, p[i], q[i]);
        }
    };

    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (nrows > 0) {
        // the first covered sample: position 0 of the recording's first beat
        const int64_t p0 = a.beat_table[4 * first] - ooff;
        double y0[8];
        truth8(p0, 1, y0);
        const double xf = (double)pred[p0], yf = y0[0];
        for (int64_t k = wave; k < nrows; k += 4) {
            const int64_t* __restrict__ bt = a.beat_table + 4 * (first + k);
            const int64_t p = bt[0] - ooff;
            const int n = (int)bt[2], cover = (a.fill || n < BL) ? n : BL;
            for (int t0 = 8 * lane; t0 < cover; t0 += 8 * 64) {
                const int nv = cover - t0 < 8 ? cover - t0 : 8;
                double x[8], y[8];
                load8(pred + p + t0, nv, ptr_align(pred + p), x);
                truth8(p + t0, nv, y);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (i < nv) {
                        const double d = x[i] - y[i], u = x[i] - xf, w = y[i] - yf;
                        s[0] += 1.0;
                        s[1] += d * d;
                        s[2] += u;
                        s[3] += w;
                        s[4] += u * u;
                        s[5] += w * w;
                        s[6] += u * w;
                    }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double w = nef_wave_sum_d(s[j]);
        if (lane == 0) red[wave][j] = w;
    }
    __syncthreads();
    if (tid < 7) res[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace

extern "C" {

size_t nef_beat_range_args_bytes(void) { return sizeof(nef_beat_range_args); }
size_t nef_beat_stitch_args_bytes(void) { return sizeof(nef_beat_stitch_args); }
size_t nef_recording_stats_args_bytes(void) { return sizeof(nef_recording_stats_args); }

int nef_beat_range(const nef_beat_range_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->signal && a->plan && a->range, NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->V >= 1 && a->V <= 12 && a->R >= 0 && a->R <= 64, NEF_E_SHAPE);
    NEF_REQUIRE((a->dtype == 0 || a->dtype == 1) && a->signal_elems >= 1 && a->signal_elems < (1ll << 56), NEF_E_SHAPE);
    NEF_REQUIRE(((uintptr_t)a->signal & 15) == 0 && (((uintptr_t)a->plan | (uintptr_t)a->range) & 7) == 0, NEF_E_UNSUPPORTED);
    if (a->dtype == 0)
        hipLaunchKernelGGL(beat_range_kernel<int16_t>, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(beat_range_kernel<float>, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

int nef_beat_stitch(const nef_beat_stitch_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->views && a->range && a->table && a->out, NEF_E_NULL);
    NEF_REQUIRE(a->Bt >= 1 && a->Bt <= 65535 && a->A >= 1 && a->A <= 65536 && (a->fill == 0 || a->fill == 1), NEF_E_SHAPE);
    NEF_REQUIRE(a->out_elems >= 1 && a->out_elems < (1ll << 40), NEF_E_SHAPE);
    // rows of 512 that neither overlap nor wrap: the angle rows of a beat first, the beats behind them
    NEF_REQUIRE(a->view_as >= BL && a->view_as < (1ll << 40) && a->view_bs >= (int64_t)a->A * a->view_as && a->view_bs < (1ll << 46), NEF_E_SHAPE);
    NEF_REQUIRE((((uintptr_t)a->views | (uintptr_t)a->out) & 3) == 0 && (((uintptr_t)a->range | (uintptr_t)a->table) & 7) == 0, NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(beat_stitch_kernel, dim3((unsigned)((a->A + 3) / 4), (unsigned)a->Bt), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

int nef_recording_stats(const nef_recording_stats_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->out && a->signal && a->beat_table && a->rec_table && a->out_offsets && a->score_leads && a->stats, NEF_E_NULL);
    NEF_REQUIRE(a->Bt >= 1 && a->N >= 1 && a->A >= 1 && a->A <= 65536 && (int64_t)a->N * a->A <= 0x7FFFFFFFll, NEF_E_SHAPE);
    NEF_REQUIRE((a->fill == 0 || a->fill == 1) && (a->dtype == 0 || a->dtype == 1), NEF_E_SHAPE);
    NEF_REQUIRE(a->out_elems >= 1 && a->out_elems < (1ll << 40) && a->signal_elems >= 1 && a->signal_elems < (1ll << 56), NEF_E_SHAPE);
    NEF_REQUIRE(((uintptr_t)a->signal & 15) == 0 && (((uintptr_t)a->out | (uintptr_t)a->score_leads) & 3) == 0, NEF_E_UNSUPPORTED);
    NEF_REQUIRE((((uintptr_t)a->beat_table | (uintptr_t)a->rec_table | (uintptr_t)a->out_offsets | (uintptr_t)a->stats) & 7) == 0, NEF_E_UNSUPPORTED);
    const dim3 grid((unsigned)((int64_t)a->N * a->A));
    if (a->dtype == 0)
        hipLaunchKernelGGL(recording_stats_kernel<int16_t>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(recording_stats_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
