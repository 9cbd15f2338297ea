// Input-lead augmentation of the train step (cfg.DATA.aug_*): white Gaussian noise, one baseline-wander and one mains-hum sinusoid per
// (sample, lead), and whole leads dropped -- y = corrupted copy of x [B, V, L], out of place.  Definition: include/nefnet_hip.h
// (nef_augment_args).  Every draw is a function of (seed, position) through nef_rng_mix, so there is no state, no atomics and one
// writer per element: the eager step, the replayed step (seed_dev) and a resumed run see the same bits.
//
// One workgroup per (row, tile of NEF_AUGMENT_TILE positions); a thread owns four neighbouring positions = one 16-byte load, one
// 16-byte store and two noise words.  The row's parameters come from blockIdx alone (wave-uniform), in fp64; the phase of a sinusoid is
// formed and reduced to [0, 1) turns in fp64 (a 50 Hz hum's 4000 turns at t = 40000 would be good to 2^-12 turns in fp32), the sine
// itself is fp32.
#include "nef_common.h"
#include "aug_drop.h"

namespace {

using namespace nef_aug;      // field0 / field1 / INV24F / ROW_BASE / lead_dropped: shared with nef_augment_mask

constexpr int TILE = NEF_AUGMENT_TILE;
static_assert(TILE == 256 * 4, "one float4 per thread of a 256-thread block");
constexpr double INV24 = 1.0 / 16777216.0;

// sin(2 pi (w t + phi)) with the phase in turns: fp64 up to the reduced phase, fp32 from there
__device__ __forceinline__ float turn_sin(double w, double phi, int t) {
    double ph = w * (double)t + phi;
    ph = ph - floor(ph);
    return sinpif(2.0f * (float)ph);
}

__global__ __launch_bounds__(256) void augment_kernel(const nef_augment_args a, int tiles) {
    const int row = (int)(blockIdx.x / (unsigned)tiles);
    const int t0 = (int)(blockIdx.x - (unsigned)row * (unsigned)tiles) * TILE + (int)threadIdx.x * 4;
    if (t0 >= a.L) return;                               // L % 4 == 0: the four positions are inside the row or all outside
    const int b = row / a.V, v = row - b * a.V;
    const uint64_t seed = a.seed + (a.seed_dev ? a.seed_dev[0] : 0ull);
    const int64_t e0 = (int64_t)row * a.L + t0;          // dense element index, a multiple of 4
    float4* __restrict__ out = reinterpret_cast<float4*>(a.y + e0);
    const uint64_t rc = ROW_BASE + 4ull * (uint64_t)row;

    if (lead_dropped(seed, b, v, a.V, a.lead_drop)) {                // block-uniform (aug_drop.h)
        *out = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }

    const float4 xv = *reinterpret_cast<const float4*>(a.x + e0);
    int end = a.L;
    if (a.crop) {
        const int64_t e = a.rois[((int64_t)b * a.R + (a.R - 1)) * 2];       // rois[b, -1, 0]
        end = e < 0 ? 0 : (e > a.L ? a.L : (int)e);
    }
    if (t0 >= end) {                                     // behind the row's end: the loader's padding stays as it is
        *out = xv;
        return;
    }
    float y[4] = {xv.x, xv.y, xv.z, xv.w};
    if (a.noise_std > 0.f) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const uint64_t z = nef_rng_mix(seed, (uint64_t)(e0 >> 1) + p);
            const float r = sqrtf(-2.0f * logf((float)(field0(z) + 1u) * INV24F));
            float s, c;
            sincospif(2.0f * ((float)field1(z) * INV24F), &s, &c);
            y[2 * p] = y[2 * p] + a.noise_std * (r * c);
            y[2 * p + 1] = y[2 * p + 1] + a.noise_std * (r * s);
        }
    }
    if (a.wander_amp > 0.0 || a.hum_amp > 0.0) {
        const uint64_t z1 = nef_rng_mix(seed, rc + 1);
        if (a.wander_amp > 0.0) {
            const uint64_t z0 = nef_rng_mix(seed, rc);
            const float A = (float)(a.wander_amp * ((double)field0(z0) * INV24));
            const double w = (a.wander_lo + (a.wander_hi - a.wander_lo) * ((double)field1(z0) * INV24)) / a.sample_rate;
            const double phi = (double)field0(z1) * INV24;
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = y[i] + A * turn_sin(w, phi, t0 + i);
        }
        if (a.hum_amp > 0.0) {
            const float A = (float)(a.hum_amp * ((double)field1(z1) * INV24));
            const double w = a.hum_hz / a.sample_rate;
            const double phi = (double)field0(nef_rng_mix(seed, rc + 2)) * INV24;
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = y[i] + A * turn_sin(w, phi, t0 + i);
        }
    }
    // a row end inside these four positions (it may split a noise pair): the positions at or behind it keep their bits
    *out = make_float4(y[0], t0 + 1 < end ? y[1] : xv.y, t0 + 2 < end ? y[2] : xv.z, t0 + 3 < end ? y[3] : xv.w);
}

}  // namespace

extern "C" {

size_t nef_augment_args_bytes(void) { return sizeof(nef_augment_args); }

int nef_augment(const nef_augment_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->x && a->y, NEF_E_NULL);
    NEF_REQUIRE(!a->crop || a->rois, NEF_E_NULL);
    NEF_REQUIRE(a->B > 0 && a->V > 0 && a->L > 0 && a->L % 4 == 0 && (!a->rois || a->R > 0), NEF_E_SHAPE);
    // (NaN fails every comparison below)
    NEF_REQUIRE(a->noise_std >= 0.f && a->wander_amp >= 0.0 && a->hum_amp >= 0.0 && a->lead_drop >= 0.f && a->lead_drop < 1.f, NEF_E_SHAPE);
    NEF_REQUIRE(a->sample_rate > 0.0, NEF_E_SHAPE);
    if (a->wander_amp > 0.0)
        NEF_REQUIRE(a->wander_lo >= 0.0 && a->wander_lo <= a->wander_hi && a->wander_hi < 0.5 * a->sample_rate, NEF_E_SHAPE);
    if (a->hum_amp > 0.0) NEF_REQUIRE(a->hum_hz >= 0.0 && a->hum_hz < 0.5 * a->sample_rate, NEF_E_SHAPE);
    const int64_t rows = (int64_t)a->B * a->V, tiles = nef_cdiv(a->L, TILE);
    NEF_REQUIRE(rows * tiles <= 0x7FFFFFFFll && rows <= 0x7FFFFFFFll, NEF_E_SHAPE);
    const uintptr_t x0 = (uintptr_t)a->x, y0 = (uintptr_t)a->y, bytes = (uintptr_t)rows * (uintptr_t)a->L * sizeof(float);
    NEF_REQUIRE(((x0 | y0) & 15) == 0 && (x0 + bytes <= y0 || y0 + bytes <= x0), NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)(rows * tiles)), dim3(256), 0, (hipStream_t)stream, *a, (int)tiles);
    return nef_launch_status();
}

}  // extern "C"
