// What the passes over an 8-bit slide share (slide.hip, stain.hip): the 4-pixel group load, the single-pixel load, the tissue rule and the
// checks of the slide's geometry.  Everything is local to the including file.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

// the PB dwords that hold the 4 pixels at p (PB bytes each, all inside the slide), shifted so that byte 0 of e[0] is p[0]
template <int PB>
__device__ __forceinline__ void load4_raw(const unsigned char* p, unsigned* e) {
    const unsigned mis = (unsigned)((uintptr_t)p & 3);
    const unsigned* q = (const unsigned*)(p - mis);
    unsigned d[PB + 1];
#pragma unroll
    for (int i = 0; i < PB; ++i) d[i] = q[i];
    d[PB] = mis ? q[PB] : 0u;                                  // the extra dword only when it holds bytes of the group
#pragma unroll
    for (int i = 0; i < PB; ++i) e[i] = __funnelshift_r(d[i], d[i + 1], mis * 8);
}

// the 4 pixels at p (PB bytes each, all inside the slide) as packed r | g << 8 | b << 16
template <int PB>
__device__ __forceinline__ void load4(const unsigned char* p, unsigned* px) {
    unsigned e[PB];
    load4_raw<PB>(p, e);
    if (PB == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = e[j] & 0xFFFFFFu;
    } else {
        px[0] = e[0] & 0xFFFFFFu;
        px[1] = (e[0] >> 24) | ((e[1] & 0xFFFFu) << 8);
        px[2] = (e[1] >> 16) | ((e[2] & 0xFFu) << 16);
        px[3] = e[2] >> 8;
    }
}

__device__ __forceinline__ unsigned load1(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }

__device__ __forceinline__ int is_tissue(unsigned px, unsigned background) {
    const unsigned r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
    const unsigned m = r < g ? (r < b ? r : b) : (g < b ? g : b);
    return m < background ? 1 : 0;
}

bool slide_args_ok(const void* slide, long long pitch, int pixel_bytes, int H, int W, const char* who) {
    if (!slide) {
        hdy_set_error("%s: null slide", who);
        return false;
    }
    if (pixel_bytes != 3 && pixel_bytes != 4) {
        hdy_set_error("%s: pixel_bytes is %d, 3 (RGB) or 4 (RGBA) expected", who, pixel_bytes);
        return false;
    }
    if (H <= 0 || W <= 0) {
        hdy_set_error("%s: slide of %d x %d pixels", who, H, W);
        return false;
    }
    if (pitch < (long long)W * pixel_bytes) {
        hdy_set_error("%s: row pitch of %lld bytes is below W * pixel_bytes = %lld", who, pitch, (long long)W * pixel_bytes);
        return false;
    }
    return true;
}

}  // namespace
