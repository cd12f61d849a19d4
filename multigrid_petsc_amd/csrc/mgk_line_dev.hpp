// mgk_line_dev.hpp -- what the line passes share (mgk_line.hip, mgk_xline.hip, mgk_line_chunk.hip, mgk_xline_chunk.hip, mgk_line_tail.hip),
// each piece stated once: the buffer windows with their out-of-range lane offset, static unrolling, the store policy, the 64 x 16 tile of the
// x marches with its LDS bank rule, and the geometry every line launcher checks first.  Nothing in here is a kernel: the kernels, their
// argument structs and their names stay in the .hip files.
#pragma once
#include "mgk_dev.hpp"
#include <type_traits>

// ---- buffer windows.  Loads and stores of the marches go through buffer descriptors: a row is a scalar byte offset, the column one constant
// VGPR, and a lane that must not load or store has a lane offset out of range -- such a load returns 0 and such a store is dropped by the
// hardware: no branch, no 64-bit vector address arithmetic.  The three constants hang together: a window never spans LINE_RECORDS bytes
// because the host refuses a pitch above LINE_MAX_PITCH, and LINE_OOB lies above LINE_RECORDS, so it is out of range in every window.
constexpr int LINE_RECORDS = 0x7ffffff0;        // every buffer window: far more than a window spans (the host checks the pitch) ...
constexpr unsigned LINE_OOB = 0x7ffffff8u;      // ... and below the lane offset of a lane that must not load or store
constexpr long LINE_MAX_PITCH = 1L << 21;       // y marches: (32 + 32 + 3) rows of a window (a period, the deepest ring, the rows around them) stay
                                                // below 2^31 bytes; x marches: 64 rows of a window and a row of 2^21 doubles stay below 2^31 bytes

typedef unsigned int line_u2 __attribute__((ext_vector_type(2)));
// a window of a field: column cb and row `row` at offset 0.  Rows are addressed by a scalar byte offset, columns by one constant VGPR.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t line_window(const double *p, int cb, long row, long rs) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)((uintptr_t)p + (uintptr_t)((cb + row * rs) * 8)), 0, LINE_RECORDS, 0x00020000);
}
// a window of a field or of a table: row `row`, column 0 at offset 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t line_window(const double *p, long row, long rs) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)((uintptr_t)p + (uintptr_t)(row * rs * 8)), 0, LINE_RECORDS, 0x00020000);
}
__device__ __forceinline__ double line_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
template <bool NT> __device__ __forceinline__ void line_st(double v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(line_u2, v), r, voff, soff, NT ? 2 : 0);
}

// ---- static unrolling: f(line_ic<K>{}) for K = K0 .. N - 1, so that K is a constant expression in f (statically indexed register rings)
template <int K> using line_ic = std::integral_constant<int, K>;
template <int K, int N> struct LineUnroll {
    template <class F> static __device__ __forceinline__ void run(F &&f) { f(line_ic<K>{}); LineUnroll<K + 1, N>::run(f); }
};
template <int N> struct LineUnroll<N, N> { template <class F> static __device__ __forceinline__ void run(F &&) {} };

// ---- the store policy of a pass, from the nt field of its argument struct (store_policy(), mgk_dev.hpp): < 0 by size, 0 ordinary, 1 non-temporal
__device__ __forceinline__ bool line_store_nt(int nt, int ny, long rs) { return nt < 0 ? mgk_store_nt_2d(ny, rs) : nt != 0; }

// ---- the tile of the x marches (mgk_xline.hip, mgk_xline_chunk.hip).  Memory stays coalesced: a step moves a TILE of 64 rows x 16 columns,
// one whole 128-byte line per row, four rows per load instruction: lane (rr, cc) = (lane / 16, lane % 16) of load k moves row 16 rr + k, column cc.
// The tile is transposed through LDS with a row pitch of 17 doubles.  By the bank rule of the 8-byte LDS accesses -- ds_read_b64: two
// groups of 32 lanes, bank pair (a / 8) mod 32; ds_write_b64: four groups of 16 contiguous lanes, bank pair (a / 8) mod 16 -- all four
// accesses are conflict-free: row-wise write and read touch (272 rr + 17 k + cc), 16 consecutive doubles per group of 16 lanes and, as
// 272 = 16 (mod 32), 32 consecutive ones per half wave; the transposed read and write touch (17 lane + c), distinct mod 32 in a half wave
// and mod 16 in 16 contiguous lanes because 17 is odd.
constexpr int XT = 16;                          // columns per tile: one 128-byte line per row
constexpr int XP = XT + 1;                      // LDS row pitch in doubles (odd: see the bank rule above)
constexpr int XTILE = 64 * XP;                  // doubles of one tile in LDS
// what the marches know about their lane: in the row-wise form of a tile lane (rr, cc) moves row r0 + 16 rr + k with load / store k
struct XLane {
    int lane, rr, cc, rq;           // rq: the row of load 0
    unsigned vf, vg;                // lane offsets (bytes) into a field window and into the table window
    unsigned rs8, gs8;
    int nx, ny;
    __device__ __forceinline__ XLane(long rs, long gs, int nx_, int ny_, int r0) {
        lane = threadIdx.x; rr = lane >> 4; cc = lane & 15; rq = r0 + 16 * rr;
        vf = (unsigned)((16 * rr * rs + cc) * 8); vg = (unsigned)((16 * rr * gs + cc) * 8);
        rs8 = (unsigned)rs * 8u; gs8 = (unsigned)gs * 8u;
        nx = nx_; ny = ny_;
    }
    __device__ __forceinline__ bool row_ok(int k) const { return (unsigned)(rq + k) < (unsigned)ny; }      // a grid row (not a ghost row)
    // an interior column of tile t, under two names: the plain backward march prefetches tile t - D and walks on to tiles t < 0, which lie
    // before the row; every other march only names tiles of the row, and the test they do not need makes three of the chunk kernels longer
    __device__ __forceinline__ bool col_ok_any(int t) const { return t >= 0 && t * XT + cc < nx; }          // any tile index
    __device__ __forceinline__ bool col_ok_nonneg(int t) const { return t * XT + cc < nx; }                 // tile index known to be >= 0
    __device__ __forceinline__ int rowwise(int k) const { return (16 * rr + k) * XP + cc; }                 // LDS index, row-wise form
    __device__ __forceinline__ int transposed(int c) const { return lane * XP + c; }                        // LDS index, lane-per-row form
};

// ---- host side: the geometry every line launcher checks before its own conditions.  A 2-D grid with at least one row and one column ...
static inline bool line_dims_ok(const mgk_geom *g) { return g && g->dim == 2 && g->nz == 1 && g->nx >= 1 && g->ny >= 1; }
// ... and, for the passes that address through windows, a pitch a window can span
static inline bool line_geom_ok(const mgk_geom *g) { return line_dims_ok(g) && g->pitch <= LINE_MAX_PITCH; }
static inline long round16(long n) { return (n + 15) / 16 * 16; }      // rows of 16 doubles: whole 128-byte lines
