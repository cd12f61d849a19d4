// mgk_launch.hpp -- the launch rules of libmgk.so's host side, each stated once (included by mgk_dev.hpp, after mgk_ctx and the tuning knobs):
// wave width and ring depth -> kernel instantiation, the cut of the marching axis into chunks, the far-plane fields of the slab launches, the stencil
// coefficients of the argument structs.  Host code only: nothing in here changes what a kernel computes.
#pragma once
#include <type_traits>
#include "mgk_pow2.h"

// ---- a run-time value picks one of a listed pack of compile-time integers: the first V of VS, in the order listed, that MATCH::ok(v, V)
// accepts, the last one for anything else.  f is called with std::integral_constant<int, V>.  The instantiations are those of the listed
// values only.
template <typename MATCH, int V0, int... VS, typename F>
static inline void with_listed(int v, F &&f) {
    if constexpr (sizeof...(VS) == 0) f(std::integral_constant<int, V0>{});
    else if (MATCH::ok(v, V0)) f(std::integral_constant<int, V0>{});
    else with_listed<MATCH, VS...>(v, f);
}
struct FitsIn { static bool ok(int v, int V) { return v <= V; } };
struct Equals { static bool ok(int v, int V) { return v == V; } };
// wave width: the runtime number of waves per row `w` picks the compile-time WX among WXS (ascending): the first one with w <= WX, the
// last one for anything wider
template <int... WXS, typename F> static inline void with_width(int w, F &&f) { with_listed<FitsIn, WXS...>(w, f); }
// ring depth of the line marches: the knob's value `d` (line_depth(), xline_depth()) picks the built D equal to it, the last one listed otherwise
template <int... DS, typename F> static inline void with_depth(int d, F &&f) { with_listed<Equals, DS...>(d, f); }
template <typename F> static inline void width_1248(int w, F &&f) { with_width<1, 2, 4, 8>(w, f); }
// whole rows: the nx + 1 elements of a row (interior + right ghost) are a whole number of wave rows (wave_row = 64 lanes x the lane's vector)
// AND that number is a block width width_1248 builds.  Only then is a block exactly one row wide, which the full-row kernel forms lean on:
// unconditional loads and stores in x, the last lane of the block as the owner of the ghost column, zero pads at the two ends of the block.
// Rows of 3, 5, 6 or 7 waves (nx = 383, 639, 767, 895 in fp64) run in the next wider block and must take the predicated forms.
static inline bool whole_rows_1248(const mgk_geom *g, int wave_row) {
    if (!g || (g->nx + 1) % wave_row != 0) return false;
    const int w = (g->nx + 1) / wave_row;
    return w == 1 || w == 2 || w == 4 || w == 8;
}
template <typename F> static inline void width_48(int w, F &&f) { with_width<4, 8>(w, f); }      // the pj2 kernels: rows of 512 / 1024 only
// LAUNCH_WX(width_1248, w, (k_foo<T, WX, 3>), nblk, stream, args...): blocks of 64 * WX threads; `kernel` names WX
#define LAUNCH_WX(pick, w, kernel, nblk, s, ...)                                                      \
    pick(w, [&](auto wx_) {                                                                           \
        constexpr int WX = decltype(wx_)::value;                                                      \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(nblk)), dim3(64 * WX), 0, s, __VA_ARGS__);         \
    })
// LAUNCH_DEPTH_ZERO(line_depths, d, zero, k_foo, grid, stream, args...): one wave per block; `kernel` is a template on <D, ZERO>
#define LAUNCH_DEPTH_ZERO(pick, d, zero, kernel, grid, s, ...)                                        \
    pick(d, [&](auto d_) {                                                                            \
        constexpr int D = decltype(d_)::value;                                                        \
        if (zero) hipLaunchKernelGGL((kernel<D, true>), grid, dim3(64), 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((kernel<D, false>), grid, dim3(64), 0, s, __VA_ARGS__);               \
    })

// ---- chunks of the marching axis.  `extent` planes (rows) are cut into `nch` chunks -- by default as many as bring `tiles` tiles to
// `target` blocks -- unless the knob g_zchunk gives the chunk length; a slab context's chunk_planes hint may ask for more, shorter chunks.
struct ChunkRule {
    int min_len;            // shortest chunk the site takes
    bool zchunk_below_min;  // an explicit g_zchunk may go below min_len
    bool even;              // length rounded up to an even number (every chunk starts on an even plane)
    bool clamp;             // never longer than the extent
    int hint_mul, hint_div; // chunk_planes hint: at least ceil(hint_mul * extent / (chunk_planes / hint_div)) chunks; hint_div 0: hint not read
};
struct Chunks { int len; long count; };
static inline Chunks cut_chunks_n(const mgk_ctx *c, int extent, long nch, const ChunkRule &r) {
    if (g_zchunk > 0) nch = (extent + g_zchunk - 1) / g_zchunk;
    else if (r.hint_div && c->chunk_planes / r.hint_div > 0) {
        const int cp = c->chunk_planes / r.hint_div;
        if (nch < (r.hint_mul * extent + cp - 1) / cp) nch = (r.hint_mul * extent + cp - 1) / cp;
    }
    int len = (int)((extent + nch - 1) / nch);
    if (r.even) len = (len + 1) & ~1;
    if (len < r.min_len && !(r.zchunk_below_min && g_zchunk > 0)) len = r.min_len;
    if (r.clamp && len > extent) len = extent;
    return {len, (long)((extent + len - 1) / len)};
}
static inline Chunks cut_chunks(const mgk_ctx *c, int extent, long tiles, long target, const ChunkRule &r) {
    return cut_chunks_n(c, extent, (tiles >= target) ? 1 : (target + tiles - 1) / tiles, r);
}

// ---- the far-plane field of a slab launch: geometry gfar = (nx, ny, 2) of the slab g, same pitch; its lo ghost plane holds what the rank
// below sent (the plane below the slab's own lo ghost), its hi ghost plane what the rank above sent
static inline bool far_geom_ok(const mgk_geom *gfar, const void *far, const mgk_geom *g) {
    return gfar && far && gfar->dim == 3 && gfar->nz == 2 && gfar->nx == g->nx && gfar->ny == g->ny && gfar->pitch == g->pitch;
}
template <typename T> static inline const T *far_lo_plane(const T *far, const mgk_geom *gfar, int has) { return has ? far + gfar->org - gfar->plane : nullptr; }
template <typename T> static inline const T *far_hi_plane(const T *far, const mgk_geom *gfar, int has) { return has ? far + gfar->org + 2 * gfar->plane : nullptr; }

// ---- stencil coefficients of an argument struct with a0 .. a6, in the struct's element type: 3-D {k-1, i-1, j-1, C, j+1, i+1, k+1},
// 2-D {i-1, j-1, C, j+1, i+1} in the slots of the same neighbours (a1, a5 stay as they are: zero)
template <typename A> static inline void set_coef7(A &a, const double *coef) {
    typedef decltype(a.a0) T;
    a.a0 = (T)coef[0]; a.a1 = (T)coef[1]; a.a2 = (T)coef[2]; a.a3 = (T)coef[3]; a.a4 = (T)coef[4]; a.a5 = (T)coef[5]; a.a6 = (T)coef[6];
}
template <typename A> static inline void set_coef5(A &a, const double *coef) {
    typedef decltype(a.a0) T;
    a.a0 = (T)coef[0]; a.a2 = (T)coef[1]; a.a3 = (T)coef[2]; a.a4 = (T)coef[3]; a.a6 = (T)coef[4];
}

// ---- the exact-FMA form of the fp64 3-D constant-coefficient kernels (madd<true>, mgk_dev.hpp): taken when ALL six off-diagonal coefficients
// {k-1, i-1, j-1, j+1, i+1, k+1} are +-2^e, e >= 0 (mgk_pow2.h) -- every level of a uniform grid with npts = 2^k + 1 -- unless
// MGK_TUNE_NO_EXACT_FMA asks for the generic form.  Two instances per kernel, not one per mask.  The results are the same doubles either way.
// Offered by the kernels where it measured no slower (k_jacobi3_3d, k_jacobi2r, k_pj2r3, k_rrrow: DESIGN.md section 4 (xix)).
static inline bool exact_fma7(const double *coef) {
    return g_variant != MGK_TUNE_NO_EXACT_FMA && coef && (mgk_coef_exact_mask(coef, 7) & 0x77u) == 0x77u;
}
// LAUNCH_WX with the kernel's last template argument EX chosen by `ex`; `kernel` names WX and EX.  T: the element type -- the exact form is
// built for double only (inside a template on T the fp32 launchers instantiate nothing new)
#define LAUNCH_WX_EX(pick, w, T, ex, kernel, nblk, s, ...)                                            \
    do {                                                                                              \
        bool done_ = false;                                                                           \
        if constexpr (sizeof(T) == 8) {                                                               \
            if (ex) { constexpr bool EX = true; LAUNCH_WX(pick, w, kernel, nblk, s, __VA_ARGS__); done_ = true; } \
        }                                                                                             \
        if (!done_) { constexpr bool EX = false; LAUNCH_WX(pick, w, kernel, nblk, s, __VA_ARGS__); }  \
    } while (0)
