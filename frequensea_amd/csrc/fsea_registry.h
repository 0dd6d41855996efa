// fsea_registry.h -- table of compiled kernel configurations (host side).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fsea_fft_core.h"

namespace fsea {

// The __global__ entry points one configuration may have.  The three compile-time-mode kernels
// serve raw int8 input (flip: the bytes are the signed samples, no XOR) with the epilogue fixed:
// the nrf_fft_process path (MAG, src/nrf.c:619-630) and the sweep tools' pixel paths (DB5 with the
// DC fix, c/fft-batch-broad.c:106-121; DB10, c/fft-batch.c:83-94).  K_U8 takes any epilogue and
// either byte convention at run time (uniform branch), K_U8_ROT adds the fused frequency shift,
// K_F32 takes f32-complex input (the NUT_BUFFER_F64 branch).
// K_U8_MAG_HALF: the MAG kernel for 50 %-overlapped frames (hop == N/2) of the sizes with one frame per workgroup (8192,
// 16384): runs of consecutive frames per workgroup, every sample loaded once (FftKernel<..., RUNS = true>).
// K_U8_MAG_WIN, K_U8_WIN, K_U8_MAG_HALF_WIN, K_U8_DB5_WIN, K_U8_DB10_WIN: the u8 kernels with the taper window fused into
// pass 0 (FftKernel<..., WIN>; fsea_plan_set_window) -- what a plan with a window launches.  K_U8_ROT_WIN, K_F32_WIN: the
// frequency-shifted and the f32-complex-input kernels with the same taper (the nrf_freq_shifter -> nrf_fft chain of
// lua/fft-shifted.lua:52-55 and nrf_fft_process' F64 branch, src/nrf.c:607-612, on a plan with a window).
enum : int { K_U8_MAG = 0, K_U8_DB5 = 1, K_U8_DB10 = 2, K_U8 = 3, K_U8_ROT = 4, K_F32 = 5, K_U8_MAG_HALF = 6,
             K_U8_MAG_WIN = 7, K_U8_WIN = 8, K_U8_MAG_HALF_WIN = 9, K_U8_DB5_WIN = 10, K_U8_DB10_WIN = 11,
             K_U8_ROT_WIN = 12, K_F32_WIN = 13, K_COUNT = 14 };

struct KernelEntry {
    int n;                 // transform size
    const char *variant;   // "" = the product configuration of this n
    int t, fpw, wg, np;
    int radix[4];
    int c0;                // samples per pass-0 load (hop must be a multiple)
    int counters;          // ticket counters: 0 = never used (single-wave frames), 1 = by launches with FftArgs::dynamic_units,
                           // 2 = by every launch (the V2 schedule and the progress-word experiments of the tuning library)
    const void *fn[K_COUNT];     // __global__ functions (launches, occupancy queries); null = not compiled
    const char *name[K_COUNT];   // symbol names as rocprof shows them
    size_t lds_bytes[K_COUNT];   // static LDS of each kind (the windowed u8 kinds that keep the DC table in LDS have it on top)
};

// Records one kind of `e`; returns true so that it can initialise a file-scope constant (FSEA_KIND_).
inline bool add_kind(KernelEntry &e, int kind, const void *fn, const char *name, size_t lds_bytes) {
    e.fn[kind] = fn;
    e.name[kind] = name;
    e.lds_bytes[kind] = lds_bytes;
    return true;
}

// Each k_*.hip translation unit exports `int fsea_kernels_<tag>(KernelEntry *out, int cap)`
// which fills `out` with its configurations and returns how many it has.

}  // namespace fsea

#define FSEA_KERNEL_FN_(NAME, SUFFIX, ...)                                                            \
    extern "C" __global__ __launch_bounds__(NAME##_cfg::WG, NAME##_cfg::WPE) void NAME##SUFFIX(       \
        fsea::FftArgs a) {                                                                            \
        __shared__ __attribute__((aligned(16))) fsea::cf lds[fsea::FftKernel<NAME##_cfg, __VA_ARGS__>::LDS_CF]; \
        fsea::FftKernel<NAME##_cfg, __VA_ARGS__>::run(a, lds);                                        \
    }

// One kind of configuration NAME: the __global__ function NAME##SUFFIX (FftKernel<NAME_cfg, __VA_ARGS__>), recorded in
// NAME_entry with its symbol name and static LDS.  The records are dynamic initialisers of this translation unit, run in
// order when the library is loaded, after NAME_entry's constant initialisation and before any fsea_kernels_<tag> call.
#define FSEA_KIND_(NAME, KIND, SUFFIX, ...)                                                           \
    FSEA_KERNEL_FN_(NAME, SUFFIX, __VA_ARGS__)                                                        \
    [[maybe_unused]] static const bool NAME##SUFFIX##_added = fsea::add_kind(                         \
        NAME##_entry, fsea::KIND, reinterpret_cast<const void *>(&NAME##SUFFIX), #NAME #SUFFIX,       \
        sizeof(fsea::cf) * fsea::FftKernel<NAME##_cfg, __VA_ARGS__>::LDS_CF);

// The kinds, each spelled once:                    kind               suffix            FftKernel<Cfg, IN, MODE_T, ROT, RUNS, WIN>
#define FSEA_K_U8_MAG_(N)             FSEA_KIND_(N, K_U8_MAG,          _u8_mag,          fsea::IN_U8,  fsea::MODE_MAG,          false, false, 0)
#define FSEA_K_U8_DB5_(N)             FSEA_KIND_(N, K_U8_DB5,          _u8_db5,          fsea::IN_U8,  fsea::MODE_DB5_U8_DCFIX, false, false, 0)
#define FSEA_K_U8_DB10_(N)            FSEA_KIND_(N, K_U8_DB10,         _u8_db10,         fsea::IN_U8,  fsea::MODE_DB10_U8,      false, false, 0)
#define FSEA_K_U8_(N)                 FSEA_KIND_(N, K_U8,              _u8,              fsea::IN_U8,  -1,                      false, false, 0)
#define FSEA_K_U8_ROT_(N)             FSEA_KIND_(N, K_U8_ROT,          _u8_rot,          fsea::IN_U8,  -1,                      true,  false, 0)
#define FSEA_K_F32_(N)                FSEA_KIND_(N, K_F32,             _f32,             fsea::IN_F32, -1,                      false, false, 0)
#define FSEA_K_U8_MAG_HALF_(N)        FSEA_KIND_(N, K_U8_MAG_HALF,     _u8_mag_half,     fsea::IN_U8,  fsea::MODE_MAG,          false, true,  0)
#define FSEA_K_U8_MAG_WIN_(N, W)      FSEA_KIND_(N, K_U8_MAG_WIN,      _u8_mag_win,      fsea::IN_U8,  fsea::MODE_MAG,          false, false, W)
#define FSEA_K_U8_DB5_WIN_(N, W)      FSEA_KIND_(N, K_U8_DB5_WIN,      _u8_db5_win,      fsea::IN_U8,  fsea::MODE_DB5_U8_DCFIX, false, false, W)
#define FSEA_K_U8_DB10_WIN_(N, W)     FSEA_KIND_(N, K_U8_DB10_WIN,     _u8_db10_win,     fsea::IN_U8,  fsea::MODE_DB10_U8,      false, false, W)
#define FSEA_K_U8_WIN_(N, W)          FSEA_KIND_(N, K_U8_WIN,          _u8_win,          fsea::IN_U8,  -1,                      false, false, W)
#define FSEA_K_U8_ROT_WIN_(N, W)      FSEA_KIND_(N, K_U8_ROT_WIN,      _u8_rot_win,      fsea::IN_U8,  -1,                      true,  false, W)
#define FSEA_K_F32_WIN_(N, W)         FSEA_KIND_(N, K_F32_WIN,         _f32_win,         fsea::IN_F32, -1,                      false, false, W)
#define FSEA_K_U8_MAG_HALF_WIN_(N, W) FSEA_KIND_(N, K_U8_MAG_HALF_WIN, _u8_mag_half_win, fsea::IN_U8,  fsea::MODE_MAG,          false, true,  W)

// The configuration NAME (FftCfg<...>) and its registry entry, which the kind lists below fill.
#define FSEA_CONFIG_(NAME, VARIANT, ...)                                                              \
    using NAME##_cfg = fsea::FftCfg<__VA_ARGS__>;                                                     \
    static fsea::KernelEntry NAME##_entry = {                                                         \
        NAME##_cfg::N, VARIANT, NAME##_cfg::T, NAME##_cfg::FPW, NAME##_cfg::WG, NAME##_cfg::NP,       \
        {NAME##_cfg::R(0), NAME##_cfg::R(1), NAME##_cfg::R(2), NAME##_cfg::R(3)}, NAME##_cfg::C(0),   \
        fsea::FftKernel<NAME##_cfg, fsea::IN_U8>::counters_used()};

// A configuration with the six kernels, with plain C names so that profiles are easy to read.  NAME: C symbol stem;
// VARIANT: registry key.
#define FSEA_DEFINE_KERNEL(NAME, VARIANT, ...)                                                        \
    FSEA_CONFIG_(NAME, VARIANT, __VA_ARGS__)                                                          \
    FSEA_K_U8_MAG_(NAME) FSEA_K_U8_DB5_(NAME) FSEA_K_U8_DB10_(NAME) FSEA_K_U8_(NAME) FSEA_K_U8_ROT_(NAME) FSEA_K_F32_(NAME)

// Tuning variants (libfsea_hip_tune.so only): the MAG kernel and the run-time-mode kernel.  The pixel modes of such a
// plan run the run-time-mode kernel; its f32-input and frequency-shifted kinds do not exist (a launch fails with
// FSEA_EINVAL).  The V2 schedule (opt::V2) always hands its frames out by the ticket pools: fsea_plan_set_unit_distribution
// has no effect on a V2 variant.
#define FSEA_DEFINE_KERNEL_LITE(NAME, VARIANT, ...)                                                   \
    FSEA_CONFIG_(NAME, VARIANT, __VA_ARGS__)                                                          \
    FSEA_K_U8_MAG_(NAME) FSEA_K_U8_(NAME)

// The u8 kernels only (MAG, DB5, DB10 with the mode fixed, and the run-time-mode kernel): configurations that have no
// f32-input or frequency-shifted form (the single-wave 64 x 64 schedule).
#define FSEA_DEFINE_KERNEL_U8(NAME, VARIANT, ...)                                                     \
    FSEA_CONFIG_(NAME, VARIANT, __VA_ARGS__)                                                          \
    FSEA_K_U8_MAG_(NAME) FSEA_K_U8_DB5_(NAME) FSEA_K_U8_DB10_(NAME) FSEA_K_U8_(NAME)

// The half-overlap MAG kernel of a configuration defined above (one frame per workgroup).
#define FSEA_DEFINE_HALF_OVERLAP(NAME) FSEA_K_U8_MAG_HALF_(NAME)

// The windowed kernels of a configuration defined above: NAME_u8_mag_win, NAME_u8_db5_win, NAME_u8_db10_win (epilogue and
// byte convention fixed at compile time, as their un-windowed twins), NAME_u8_win, NAME_u8_rot_win, NAME_f32_win, and with
// FSEA_DEFINE_HALF_OVERLAP_WIN NAME_u8_mag_half_win.  WMODE: FftKernel's WIN (1 = weights fetched per frame,
// 2 = register-resident).
#define FSEA_DEFINE_WINDOWED(NAME, WMODE)                                                             \
    FSEA_K_U8_MAG_WIN_(NAME, WMODE) FSEA_K_U8_DB5_WIN_(NAME, WMODE) FSEA_K_U8_DB10_WIN_(NAME, WMODE)  \
    FSEA_K_U8_WIN_(NAME, WMODE) FSEA_K_U8_ROT_WIN_(NAME, WMODE) FSEA_K_F32_WIN_(NAME, WMODE)
#define FSEA_DEFINE_HALF_OVERLAP_WIN(NAME, WMODE) FSEA_K_U8_MAG_HALF_WIN_(NAME, WMODE)

// The registry list of a translation unit: FSEA_REGISTER(NAME) adds NAME_entry with every kind defined for NAME.
#define FSEA_REGISTER_BEGIN(TAG)                                                                      \
    extern "C" int fsea_kernels_##TAG(fsea::KernelEntry *out, int cap) {                              \
        int n = 0;
#define FSEA_REGISTER(NAME) if (n < cap) out[n++] = NAME##_entry;
#define FSEA_REGISTER_END                                                                             \
        return n;                                                                                     \
    }
