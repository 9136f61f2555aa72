// Event detection over recordings (ABI 16): one score per (window, class) -> events "class c is present in windows first .. last of
// sequence r, peak p".  The reference names the step and leaves it empty (avex/preprocessing/activity_detector.py has no body).
//
// Every decision is a compare of fp32 numbers; no transcendental runs here.  Time is cut into CHUNKS of EV_K = 256 consecutive global
// windows (four ROWS of 64: one row of one class is one 64-bit ballot word), whatever the sequences are: a sequence may start and end
// anywhere inside a chunk and many short ones share a chunk.  Nothing crosses a sequence boundary: a sequence's first window composes
// "inactive" in front of its own function, and every stencil is clipped to the [lo, hi) of its window's sequence.
//
//   ev_classify_kernel   (chunk, tile of <= 16 classes): the scores of 256 + 2 h windows x the tile's classes go through LDS (global reads
//                        run along classes, then windows: whole rows of the tile; LDS is class-major so thread t = window t reads
//                        conflict-free).  Smoothing, then per window "set" (s >= on) / "clear" (!(s >= off), or a hold in a sequence's
//                        first window): two ballot words per (row, class), and the chunk's composed function {hold, const 0, const 1}.
//   ev_carry_kernel      one workgroup per class: the state entering every chunk, a scan of the composed functions 256 chunks at a time
//                        (the last set / clear below a lane decides; ballots, no atomics).
//   ev_runs_kernel       (chunk, class): replays the state into active words for the chunk's rows and two rows of halo on each side,
//                        fills gaps (nearest active window on either side from clz / ctz of a 64-bit view: merge_gap <= 64), then drops
//                        short runs (length from the runs of "linked to the window before" bits, min_windows <= 64).  Writes the final
//                        active word, the event-start word and the chunk's number of starts.
//   ev_count_kernel      one workgroup per class: exclusive prefix of the starts over the chunks.
//   ev_bounds_kernel     one workgroup per sequence boundary x = off[r]: P_c(x) = starts of class c below x, its exclusive prefix over
//                        the classes V[r][c] and the sum T[r].  An event (r, c, first) is then number
//                            T[r] + (V[r + 1][c] - V[r][c]) + P_c(first) - P_c(off[r])
//                        in the order (sequence, class, first): a count of the events in front of it, no sort, no atomics.  T[R] is the total.
//   ev_emit_kernel       (chunk, tile): smooths again (the smoothed scores are never stored), writes sequence / class / first from the
//                        start bits and last from the end bits, and reduces every run SEGMENT inside the chunk (its first thread walks at
//                        most the chunk): a run that starts and ends here is written; otherwise the segment is the chunk's "in" partial
//                        (enters from the chunk before: ends here, or runs through) or "out" partial (starts here, leaves).
//   ev_join_kernel       (chunk, class) with an out partial: 256 threads take the following chunks' in partials 256 at a time up to the
//                        first that ends, and reduce them in a fixed order.  peak / peak_window are order-free (max, lowest window);
//                        the fp64 sum adds per-chunk partials, so its bits depend on where the chunk boundaries fall in the event.
//   ev_fill_kernel       rows past min(total, capacity): -1, -inf, NaN.
#include <math.h>

#include "block_prims.h"
#include "common.h"

namespace {

constexpr int EV_K = 256;              // windows of one chunk = threads of a workgroup
constexpr int EV_ROWS = EV_K / 64;     // ballot words of one chunk and class
constexpr int EV_TC = 16;              // classes of one score tile
constexpr int EV_MAX_SMOOTH = 31;
constexpr int EV_MAX_SPAN = 64;        // merge_gap and min_windows: what one 64-bit view on either side can decide
constexpr int EV_LDW = EV_K + EV_MAX_SMOOTH;      // LDS floats of one class of a tile (odd: the fill's stride hits every bank)
constexpr int64_t EV_MAX_WINDOWS = 0x7fffffffll;
constexpr int64_t EV_MAX_BLOCKS = 0x7fffffffll;

typedef unsigned long long u64;

struct EvPart {            // a run segment's reduction; cnt = 0: no non-NaN score seen yet
    double sum;
    long long rank;        // out partials: the event's number (-1: beyond the capacity, nobody joins it)
    float mx;
    int arg;               // global window of mx, the lowest
    int cnt;
    int flag;              // in partials: 0 none, 1 the run ends in this chunk, 2 it runs through;  out partials: 1 present
};

struct EvWs {
    u64* S;                // [C][rows]  set bits
    u64* Z;                //            clear bits
    u64* F;                //            final active bits
    u64* E;                //            event-start bits
    int* pch;              // [C][chunks + 1]  starts per chunk, then their exclusive prefix; [chunks] = the class's total
    long long* V;          // [R + 1][C]
    long long* T;          // [R + 1]
    EvPart* pin;           // [C][chunks]
    EvPart* pout;          // [C][chunks]
    unsigned char* summ;   // [C][chunks]  0 hold, 1 const 0, 2 const 1
    unsigned char* carry;  // [C][chunks]  state entering the chunk
    size_t bytes;
};

static EvWs ev_carve(void* ws, int64_t n, int64_t c, int64_t r) {
    const size_t nch = (size_t)((n + EV_K - 1) / EV_K), rows = nch * EV_ROWS, C = (size_t)c;
    const size_t step = 16;      // bytes: every array starts 16-byte aligned
    EvWs w;
    char* p = (char*)ws;
    w.S = take<u64>(p, C * rows, step);
    w.Z = take<u64>(p, C * rows, step);
    w.F = take<u64>(p, C * rows, step);
    w.E = take<u64>(p, C * rows, step);
    w.pch = take<int>(p, C * (nch + 1), step);
    w.V = take<long long>(p, (size_t)(r + 1) * C, step);
    w.T = take<long long>(p, (size_t)(r + 1), step);
    w.pin = take<EvPart>(p, C * nch, step);
    w.pout = take<EvPart>(p, C * nch, step);
    w.summ = take<unsigned char>(p, C * nch, step);
    w.carry = take<unsigned char>(p, C * nch, step);
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

struct EvParams {
    const float* scores;
    int64_t ld;
    int64_t M;
    int N, C, R;
    int nch, ntile;
    const int64_t* off;            // [R + 1] on the device
    const int32_t* rowmap;         // [N] or NULL
    const float* on;
    const float* offt;
    int h, mode, gap, minw;
    EvWs w;
    long long* total;
    // emit
    long long cap;
    int32_t* o_seq;
    int32_t* o_cls;
    int32_t* o_first;
    int32_t* o_last;
    float* o_peak;
    int32_t* o_peakw;
    double* o_mean;
};

// the sequence of window i (0 <= i < N): the r with off[r] <= i < off[r + 1]; off[0] = 0 and off[R] = N hold the invariant
static __device__ __forceinline__ int ev_seq_of(const int64_t* __restrict__ off, int R, int64_t i) {
    int l = 0, h = R;
    while (h - l > 1) {
        const int m = l + ((h - l) >> 1);
        if (off[m] <= i) l = m; else h = m;
    }
    return l;
}

// the last set / clear decides: the words are disjoint, so the higher top bit is the larger number
static __device__ __forceinline__ int ev_apply(int st, u64 s, u64 z) { return (s | z) ? (s > z ? 1 : 0) : st; }

// scores of windows i0 - h .. i0 + 255 + h x classes c0 .. c0 + tc - 1 -> raw[cc * EV_LDW + w]; no score (outside 0 .. N - 1, a row
// of -1 or outside the matrix): NaN.  Consecutive threads read consecutive classes of one window, then the next window.
static __device__ __forceinline__ void ev_load_tile(const EvParams& p, int64_t i0, int c0, int tc, float* raw) {
    const int span = EV_K + 2 * p.h;
    for (int idx = threadIdx.x; idx < span * tc; idx += EV_K) {
        const int w = idx / tc, cc = idx - w * tc;
        const int64_t i = i0 - p.h + w;
        float v = __builtin_nanf("");
        if (i >= 0 && i < p.N) {
            const int64_t row = p.rowmap ? (int64_t)p.rowmap[i] : i;
            if (row >= 0 && row < p.M) v = p.scores[row * p.ld + (int64_t)(c0 + cc)];
        }
        raw[cc * EV_LDW + w] = v;
    }
}

// v[0] is window i; the positions i - h .. i + h inside [lo, hi) that hold a number take part
static __device__ __forceinline__ float ev_smooth(const float* v, int64_t i, int64_t lo, int64_t hi, int h, int mode) {
    if (h == 0) return v[0];
    const int a = (int)((i - h > lo ? i - h : lo) - i), b = (int)((i + h < hi - 1 ? i + h : hi - 1) - i);
    if (mode == 1) {                                  // mean: the fp32 sum in position order over float(n)
        float sum = 0.f;
        int n = 0;
        for (int d = a; d <= b; ++d) {
            const float x = v[d];
            if (x == x) { sum += x; ++n; }
        }
        return n ? sum / (float)n : __builtin_nanf("");
    }
    int n = 0;
    for (int d = a; d <= b; ++d) n += v[d] == v[d] ? 1 : 0;
    if (n == 0) return __builtin_nanf("");
    const int k = (n - 1) >> 1;                       // the lower median: element k of the sorted numbers
    for (int d = a; d <= b; ++d) {
        const float x = v[d];
        if (!(x == x)) continue;
        int lt = 0, le = 0;
        for (int e = a; e <= b; ++e) {
            const float y = v[e];
            lt += y < x ? 1 : 0;
            le += y <= x ? 1 : 0;
        }
        if (lt <= k && k < le) return x;
    }
    return __builtin_nanf("");                        // not reached: some number has rank k
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Thread t owns window chunk * 256 + t for every class of the tile; wave w owns row chunk * 4 + w: its ballots are the row's words.
__global__ __launch_bounds__(EV_K) void ev_classify_kernel(EvParams p) {
    __shared__ float raw[EV_TC * EV_LDW];
    __shared__ u64 wS[EV_TC][EV_ROWS], wZ[EV_TC][EV_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / p.ntile, tile = blockIdx.x - chunk * p.ntile;
    const int c0 = tile * EV_TC, tc = p.C - c0 < EV_TC ? p.C - c0 : EV_TC;
    const int64_t i0 = (int64_t)chunk * EV_K, i = i0 + tid;
    ev_load_tile(p, i0, c0, tc, raw);
    const bool inside = i < p.N;
    int64_t lo = 0, hi = 0;
    if (inside) {
        const int r = ev_seq_of(p.off, p.R, i);
        lo = p.off[r];
        hi = p.off[r + 1];
    }
    __syncthreads();
    const size_t rows = (size_t)p.nch * EV_ROWS;
    for (int cc = 0; cc < tc; ++cc) {
        const int c = c0 + cc;
        bool set = false, clr = false;
        if (inside) {
            const float s = ev_smooth(raw + cc * EV_LDW + p.h + tid, i, lo, hi, p.h, p.mode);
            set = s >= p.on[c];
            clr = !(s >= p.offt[c]) || (i == lo && !set);      // a sequence starts inactive: a hold in its first window is a clear
        }
        const u64 bs = __ballot(set), bz = __ballot(clr);
        if (lane == 0) {
            const size_t at = (size_t)c * rows + (size_t)chunk * EV_ROWS + wave;
            p.w.S[at] = bs;
            p.w.Z[at] = bz;
            wS[cc][wave] = bs;
            wZ[cc][wave] = bz;
        }
    }
    __syncthreads();
    if (tid < tc) {                                   // thread cc composes the four rows of class c0 + cc
        int code = 0;
#pragma unroll
        for (int w = 0; w < EV_ROWS; ++w) {
            const u64 s = wS[tid][w], z = wZ[tid][w];
            if (s | z) code = s > z ? 2 : 1;
        }
        p.w.summ[(size_t)(c0 + tid) * p.nch + chunk] = (unsigned char)code;
    }
}

// One workgroup per class; thread t owns chunk base + t of the pass.
__global__ __launch_bounds__(EV_K) void ev_carry_kernel(EvParams p) {
    __shared__ u64 wS[EV_ROWS], wZ[EV_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t c = blockIdx.x;
    int state = 0;                                    // entering chunk `base`
    for (int base = 0; base < p.nch; base += EV_K) {
        const int k = base + tid;
        const int code = k < p.nch ? p.w.summ[c * p.nch + k] : 0;
        const u64 bs = __ballot(code == 2), bz = __ballot(code == 1);
        if (lane == 0) { wS[wave] = bs; wZ[wave] = bz; }
        __syncthreads();
        int st = state, all = state;
#pragma unroll
        for (int w = 0; w < EV_ROWS; ++w) {
            if (w < wave) st = ev_apply(st, wS[w], wZ[w]);
            all = ev_apply(all, wS[w], wZ[w]);
        }
        const u64 below = (1ull << lane) - 1ull;
        st = ev_apply(st, bs & below, bz & below);
        if (k < p.nch) p.w.carry[c * p.nch + k] = (unsigned char)st;
        state = all;
        __syncthreads();                              // wS / wZ are rewritten by the next pass
    }
}

// One workgroup per (chunk, class).  A[q] is the active word of row chunk * 4 - 2 + q, Mw / Bw[q] the merged and sequence-start
// words of row chunk * 4 - 1 + q; a wave owns the rows it ballots.
__global__ __launch_bounds__(EV_K) void ev_runs_kernel(EvParams p) {
    __shared__ u64 A[EV_ROWS + 4], Mw[EV_ROWS + 2], Bw[EV_ROWS + 2];
    __shared__ int wcount[EV_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / p.C, c = blockIdx.x - chunk * p.C;
    const int64_t rows = (int64_t)p.nch * EV_ROWS, row0 = (int64_t)chunk * EV_ROWS;
    const u64* __restrict__ S = p.w.S + (size_t)c * rows;
    const u64* __restrict__ Z = p.w.Z + (size_t)c * rows;

    for (int q = wave; q < EV_ROWS + 4; q += EV_ROWS) {
        const int64_t row = row0 - 2 + q;
        u64 word = 0ull;
        if (row >= 0 && row < rows) {                 // wave-uniform
            const int64_t ch = row / EV_ROWS;
            int st = p.w.carry[(size_t)c * p.nch + ch];
            for (int64_t r = ch * EV_ROWS; r < row; ++r) st = ev_apply(st, S[r], Z[r]);
            const u64 upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
            const int a = ev_apply(st, S[row] & upto, Z[row] & upto);
            word = __ballot(a != 0 && row * 64 + lane < p.N);
        }
        if (lane == 0) A[q] = word;
    }
    __syncthreads();

    for (int q = wave; q < EV_ROWS + 2; q += EV_ROWS) {
        const int64_t row = row0 - 1 + q, i = row * 64 + lane;
        bool m = false, first = false;
        if (row >= 0 && i < p.N) {
            const int r = ev_seq_of(p.off, p.R, i);
            const int64_t lo = p.off[r], hi = p.off[r + 1];
            first = i == lo;
            m = (A[q + 1] >> lane) & 1ull;
            if (!m && p.gap > 0) {
                // before: windows i - 64 .. i - 1, the top bit is i - 1;  after: windows i + 1 .. i + 64, bit 0 is i + 1
                const u64 before = lane == 0 ? A[q] : (A[q + 1] << (64 - lane)) | (A[q] >> lane);
                const u64 after = lane == 63 ? A[q + 2] : (A[q + 1] >> (lane + 1)) | (A[q + 2] << (63 - lane));
                if (before != 0ull && after != 0ull) {
                    const int dl = __clzll((long long)before) + 1, dr = __ffsll((long long)after);
                    m = dl + dr - 1 <= p.gap && i - dl >= lo && i + dr < hi;      // both neighbours in this window's sequence
                }
            }
        }
        const u64 bm = __ballot(m), bb = __ballot(first);
        if (lane == 0) { Mw[q] = bm; Bw[q] = bb; }
    }
    __syncthreads();

    {
        const int q = wave + 1;
        // link bit j of a row: window j is merged-active, so is the window before it, and j does not start a sequence
        const u64 lprev = Mw[q - 1] & ((Mw[q - 1] << 1) | (q >= 2 ? Mw[q - 2] >> 63 : 0ull)) & ~Bw[q - 1];      // its bit 0 is never looked at
        const u64 lcur = Mw[q] & ((Mw[q] << 1) | (Mw[q - 1] >> 63)) & ~Bw[q];
        const u64 lnext = Mw[q + 1] & ((Mw[q + 1] << 1) | (Mw[q] >> 63)) & ~Bw[q + 1];
        const u64 down = lane == 63 ? lcur : (lcur << (63 - lane)) | (lprev >> (lane + 1));      // links of i, i - 1, ... from the top bit
        const u64 up = lane == 63 ? lnext : (lcur >> (lane + 1)) | (lnext << (63 - lane));        // links of i + 1, i + 2, ... from bit 0
        const int nl = ~down == 0ull ? 64 : __clzll((long long)~down);
        const int nr = ~up == 0ull ? 64 : __ffsll((long long)~up) - 1;
        const bool m = (Mw[q] >> lane) & 1ull;
        const bool f = m && 1 + nl + nr >= p.minw;                                              // 64 or more saturates: min_windows <= 64
        const bool start = f && !((lcur >> lane) & 1ull);
        const u64 bf = __ballot(f), be = __ballot(start);
        if (lane == 0) {
            p.w.F[(size_t)c * rows + row0 + wave] = bf;
            p.w.E[(size_t)c * rows + row0 + wave] = be;
            wcount[wave] = __popcll(be);
        }
    }
    __syncthreads();
    if (tid == 0) p.w.pch[(size_t)c * (p.nch + 1) + chunk] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

// One workgroup per class: starts per chunk -> starts in the chunks before; entry [chunks] = the class's total.
__global__ __launch_bounds__(EV_K) void ev_count_kernel(EvParams p) {
    __shared__ int wt[EV_ROWS];
    int* __restrict__ cnt = p.w.pch + (size_t)blockIdx.x * (p.nch + 1);
    int carry = 0;
    for (int base = 0; base < p.nch; base += EV_K) {
        const int k = base + threadIdx.x;
        const int v = k < p.nch ? cnt[k] : 0;
        int excl, all;
        const int incl = block_scan<EV_ROWS>(v, 0, BlockSum(), wt, &excl, &all);
        if (k < p.nch) cnt[k] = carry + incl - v;      // (incl - v, not excl: a subtraction where excl costs one more shuffle)
        carry += all;
    }
    if (threadIdx.x == 0) cnt[p.nch] = carry;
}

// event starts of class c in the windows below x (0 <= x <= N): the chunk's prefix, the whole rows of the chunk below x, the bits below x
static __device__ __forceinline__ int ev_starts_below(const EvParams& p, int c, int64_t x) {
    const int64_t rows = (int64_t)p.nch * EV_ROWS, ch = x / EV_K, row = x >> 6;
    const u64* __restrict__ E = p.w.E + (size_t)c * rows;
    int n = p.w.pch[(size_t)c * (p.nch + 1) + ch];
    for (int64_t r = ch * EV_ROWS; r < row; ++r) n += __popcll(E[r]);
    const int b = (int)(x & 63);
    if (b) n += __popcll(E[row] & ((1ull << b) - 1ull));
    return n;
}

// the number of the event of class c that starts (or, with x = last + 1 and minus one, ends) in sequence r: see the head of the file
static __device__ __forceinline__ long long ev_rank(const EvParams& p, int r, int c, int64_t lo, int64_t first) {
    const long long* __restrict__ V = p.w.V;
    return p.w.T[r] + (V[(size_t)(r + 1) * p.C + c] - V[(size_t)r * p.C + c]) + (long long)(ev_starts_below(p, c, first) - ev_starts_below(p, c, lo));
}

// One workgroup per sequence boundary r = 0 .. R; thread t owns class base + t of the pass.
__global__ __launch_bounds__(EV_K) void ev_bounds_kernel(EvParams p) {
    __shared__ long long wt[EV_ROWS];
    const int r = blockIdx.x;
    int64_t x = p.off[r];
    x = x < 0 ? 0 : (x > p.N ? p.N : x);              // the host checked its copy; a device copy that differs cannot leave the words
    long long carry = 0;
    for (int base = 0; base < p.C; base += EV_K) {
        const int c = base + threadIdx.x;
        const long long g = c < p.C ? (long long)ev_starts_below(p, c, x) : 0ll;
        long long excl, all;
        const long long incl = block_scan<EV_ROWS>(g, 0ll, BlockSum(), wt, &excl, &all);
        if (c < p.C) p.w.V[(size_t)r * p.C + c] = carry + incl - g;
        carry += all;
    }
    if (threadIdx.x == 0) {
        p.w.T[r] = carry;
        if (r == p.R) *p.total = carry;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// a number this call writes: 0 <= rank < capacity (a device copy of the offsets that differs from the checked one cannot leave the columns)
static __device__ __forceinline__ bool ev_in_cap(const EvParams& p, long long rank) { return (unsigned long long)rank < (unsigned long long)p.cap; }

static __device__ __forceinline__ void ev_part_merge(EvPart& a, const EvPart& b) {      // sums in call order; max with the lowest window
    if (b.cnt > 0 && (a.cnt == 0 || b.mx > a.mx || (b.mx == a.mx && b.arg < a.arg))) { a.mx = b.mx; a.arg = b.arg; }
    a.sum += b.sum;
    a.cnt += b.cnt;
}

// Thread t owns window chunk * 256 + t for every class of the tile: its start bit writes sequence / class / first, its end bit last.
// The first thread of a run segment (thread 0 of an active window, or a start bit) reduces the segment: at most this chunk's windows.
__global__ __launch_bounds__(EV_K) void ev_emit_kernel(EvParams p) {
    __shared__ float raw[EV_TC * EV_LDW];
    __shared__ float sm[EV_K];
    __shared__ u64 Fw[EV_ROWS + 1], Ew[EV_ROWS + 1];           // [4]: the next chunk's first row (0 past the end)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / p.ntile, tile = blockIdx.x - chunk * p.ntile;
    const int c0 = tile * EV_TC, tc = p.C - c0 < EV_TC ? p.C - c0 : EV_TC;
    const int64_t i0 = (int64_t)chunk * EV_K, i = i0 + tid;
    const int64_t rows = (int64_t)p.nch * EV_ROWS, row0 = (int64_t)chunk * EV_ROWS;
    ev_load_tile(p, i0, c0, tc, raw);
    const bool inside = i < p.N;
    int r = 0;
    int64_t lo = 0, hi = 0;
    if (inside) {
        r = ev_seq_of(p.off, p.R, i);
        lo = p.off[r];
        hi = p.off[r + 1];
    }
    for (int cc = 0; cc < tc; ++cc) {
        const int c = c0 + cc;
        __syncthreads();                              // the tile is loaded; the pass before has read sm, Fw and Ew
        sm[tid] = inside ? ev_smooth(raw + cc * EV_LDW + p.h + tid, i, lo, hi, p.h, p.mode) : __builtin_nanf("");
        if (tid <= EV_ROWS) {
            const bool have = row0 + tid < rows;
            Fw[tid] = have ? p.w.F[(size_t)c * rows + row0 + tid] : 0ull;
            Ew[tid] = have ? p.w.E[(size_t)c * rows + row0 + tid] : 0ull;
        }
        __syncthreads();
        const bool f = (Fw[wave] >> lane) & 1ull, e = (Ew[wave] >> lane) & 1ull;
        const bool leaves = (Fw[EV_ROWS] & 1ull) && !(Ew[EV_ROWS] & 1ull);      // the run of window 255, if any, goes on in the next chunk
        const int t1 = tid + 1;
        const bool goes_on = t1 < EV_K ? ((Fw[t1 >> 6] >> (t1 & 63)) & 1ull) && !((Ew[t1 >> 6] >> (t1 & 63)) & 1ull) : leaves;
        EvPart* pin = p.w.pin + (size_t)c * p.nch + chunk;
        EvPart* pout = p.w.pout + (size_t)c * p.nch + chunk;
        long long rank = -1;
        if (e) {
            rank = ev_rank(p, r, c, lo, i);
            if (ev_in_cap(p, rank)) {
                p.o_seq[rank] = r;
                p.o_cls[rank] = c;
                p.o_first[rank] = (int32_t)i;
            }
        }
        if (f && !goes_on) {
            const long long re = ev_rank(p, r, c, lo, i + 1) - 1;      // the starts up to and including i, less this event's own
            if (ev_in_cap(p, re)) p.o_last[re] = (int32_t)i;
        }
        if (tid == 0 && !(f && !e)) pin->flag = 0;                     // no run enters this chunk
        if (tid == EV_K - 1 && !(f && leaves)) pout->flag = 0;         // no run leaves it
        if (f && (tid == 0 || e)) {
            EvPart a;
            a.sum = 0.0; a.rank = -1; a.mx = -__builtin_inff(); a.arg = -1; a.cnt = 0; a.flag = 0;
            int t = tid;
            do {
                const float x = sm[t];
                if (x == x) {
                    if (a.cnt == 0 || x > a.mx) { a.mx = x; a.arg = (int)(i0 + t); }
                    a.sum += (double)x;
                    ++a.cnt;
                }
                ++t;
            } while (t < EV_K && ((Fw[t >> 6] >> (t & 63)) & 1ull) && !((Ew[t >> 6] >> (t & 63)) & 1ull));
            const bool ends = t < EV_K || !leaves;
            if (e && ends) {
                if (ev_in_cap(p, rank)) {
                    p.o_peak[rank] = a.mx;
                    p.o_peakw[rank] = a.arg;
                    p.o_mean[rank] = a.sum / (double)a.cnt;
                }
            } else if (e) {
                a.rank = ev_in_cap(p, rank) ? rank : -1;
                a.flag = 1;
                *pout = a;
            } else {
                a.flag = ends ? 1 : 2;
                *pin = a;
                if (!ends) pout->flag = 0;            // the run that leaves did not start here: nothing to join from this chunk
            }
        }
    }
}

// One workgroup per (chunk, class) that holds an out partial: thread t owns chunk base + t of the pass over the chunks that follow.
__global__ __launch_bounds__(EV_K) void ev_join_kernel(EvParams p) {
    __shared__ u64 wend[EV_ROWS];
    __shared__ EvPart wpart[EV_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k0 = blockIdx.x / p.C, c = blockIdx.x - k0 * p.C;
    const EvPart* __restrict__ pin = p.w.pin + (size_t)c * p.nch;
    const EvPart head = p.w.pout[(size_t)c * p.nch + k0];
    if (head.flag != 1 || !ev_in_cap(p, head.rank)) return;      // workgroup-uniform
    EvPart a;
    a.sum = 0.0; a.rank = -1; a.mx = -__builtin_inff(); a.arg = -1; a.cnt = 0; a.flag = 0;
    for (int base = k0 + 1; base < p.nch; base += EV_K) {
        const int k = base + tid;
        EvPart b;
        b.flag = 1;                                   // past the last chunk: an end (never reached: a run that leaves enters the next chunk)
        b.cnt = 0; b.sum = 0.0; b.mx = 0.f; b.arg = -1;
        if (k < p.nch) b = pin[k];
        const u64 be = __ballot(b.flag != 2);
        if (lane == 0) wend[wave] = be;
        __syncthreads();
        int end_at = EV_K;                            // the pass's first chunk in which the run ends
#pragma unroll
        for (int w = EV_ROWS - 1; w >= 0; --w)
            if (wend[w] != 0ull) end_at = w * 64 + __ffsll((long long)wend[w]) - 1;
        if (tid <= end_at) ev_part_merge(a, b);
        __syncthreads();                              // wend is rewritten by the next pass
        if (end_at < EV_K) break;                     // workgroup-uniform
    }
    // lanes by a butterfly (a + b == b + a bit for bit and the max rule is symmetric: every lane ends with the same record), then the waves
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        EvPart b;
        b.sum = __shfl_xor(a.sum, o, 64);
        b.mx = __shfl_xor(a.mx, o, 64);
        b.arg = __shfl_xor(a.arg, o, 64);
        b.cnt = __shfl_xor(a.cnt, o, 64);
        ev_part_merge(a, b);
    }
    if (lane == 0) wpart[wave] = a;
    __syncthreads();
    if (tid == 0) {
        EvPart lo2 = wpart[0], hi2 = wpart[2], all = head;
        ev_part_merge(lo2, wpart[1]);
        ev_part_merge(hi2, wpart[3]);
        ev_part_merge(lo2, hi2);
        ev_part_merge(all, lo2);
        p.o_peak[head.rank] = all.mx;
        p.o_peakw[head.rank] = all.arg;
        p.o_mean[head.rank] = all.sum / (double)all.cnt;
    }
}

__global__ __launch_bounds__(EV_K) void ev_fill_kernel(EvParams p) {
    const long long j = (long long)blockIdx.x * EV_K + threadIdx.x;
    if (j >= p.cap || j < *p.total) return;
    p.o_seq[j] = -1;
    p.o_cls[j] = -1;
    p.o_first[j] = -1;
    p.o_last[j] = -1;
    p.o_peak[j] = -__builtin_inff();
    p.o_peakw[j] = -1;
    p.o_mean[j] = __builtin_nan("");
}

static bool ev_shape_ok(int64_t n, int64_t c, int64_t r) {
    if (n < 1 || n > EV_MAX_WINDOWS || c < 1 || c > 0x7fffffffll || r < 1 || r > 0x7ffffffell) return false;
    const int64_t nch = (n + EV_K - 1) / EV_K;
    return nch <= EV_MAX_BLOCKS / c;                  // one workgroup per (chunk, class)
}

// what scan and emit refuse alike; fills the launch parameters
static int ev_check(const char* what, const avexhip_events_args* a, EvParams* p) {
    AVX_REQUIRE(a && a->scores && a->seq_offsets_host && a->seq_offsets_dev && a->on && a->off && a->workspace && a->total, "%s: null argument", what);
    AVX_REQUIRE(a->n_windows <= EV_MAX_WINDOWS, "%s: n_windows %lld > 2^31 - 1", what, (long long)a->n_windows);
    AVX_REQUIRE(ev_shape_ok(a->n_windows, a->n_classes, a->n_seq), "%s: bad shape (n_windows %lld, n_classes %d, n_seq %d)", what, (long long)a->n_windows,
                a->n_classes, a->n_seq);
    AVX_REQUIRE(a->n_rows >= 1 && a->ld_scores >= a->n_classes, "%s: bad score matrix (n_rows %lld, ld_scores %lld < n_classes %d)", what, (long long)a->n_rows,
                (long long)a->ld_scores, a->n_classes);
    AVX_REQUIRE(a->row_of_window || a->n_rows == a->n_windows, "%s: n_rows %lld != n_windows %lld without row_of_window", what, (long long)a->n_rows,
                (long long)a->n_windows);
    AVX_REQUIRE(a->smooth >= 1 && a->smooth <= EV_MAX_SMOOTH && (a->smooth & 1), "%s: smooth %d is not odd in 1 .. %d", what, a->smooth, EV_MAX_SMOOTH);
    AVX_REQUIRE(a->smooth_mode == 0 || a->smooth_mode == 1, "%s: smooth_mode %d is neither 0 (median) nor 1 (mean)", what, a->smooth_mode);
    AVX_REQUIRE(a->merge_gap >= 0 && a->merge_gap <= EV_MAX_SPAN, "%s: merge_gap %d outside 0 .. %d", what, a->merge_gap, EV_MAX_SPAN);
    AVX_REQUIRE(a->min_windows >= 1 && a->min_windows <= EV_MAX_SPAN, "%s: min_windows %d outside 1 .. %d", what, a->min_windows, EV_MAX_SPAN);
    const int64_t* off = a->seq_offsets_host;
    AVX_REQUIRE(off[0] == 0, "%s: seq_offsets[0] = %lld, not 0", what, (long long)off[0]);
    for (int r = 0; r < a->n_seq; ++r)
        AVX_REQUIRE(off[r + 1] >= off[r], "%s: seq_offsets[%d] = %lld < seq_offsets[%d] = %lld", what, r + 1, (long long)off[r + 1], r, (long long)off[r]);
    AVX_REQUIRE(off[a->n_seq] == a->n_windows, "%s: seq_offsets[%d] = %lld, not n_windows %lld", what, a->n_seq, (long long)off[a->n_seq],
                (long long)a->n_windows);
    const EvWs w = ev_carve(a->workspace, a->n_windows, a->n_classes, a->n_seq);
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("%s: workspace %zu B < %zu B", what, a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    memset(p, 0, sizeof(*p));
    p->scores = a->scores;
    p->ld = a->ld_scores;
    p->M = a->n_rows;
    p->N = (int)a->n_windows;
    p->C = a->n_classes;
    p->R = a->n_seq;
    p->nch = (int)((a->n_windows + EV_K - 1) / EV_K);
    p->ntile = (a->n_classes + EV_TC - 1) / EV_TC;
    p->off = a->seq_offsets_dev;
    p->rowmap = a->row_of_window;
    p->on = a->on;
    p->offt = a->off;
    p->h = (a->smooth - 1) / 2;
    p->mode = a->smooth_mode;
    p->gap = a->merge_gap;
    p->minw = a->min_windows;
    p->w = w;
    p->total = (long long*)a->total;
    return AVEXHIP_OK;
}

}  // namespace

extern "C" int avexhip_events_max_smooth(void) { return EV_MAX_SMOOTH; }
extern "C" int avexhip_events_max_span(void) { return EV_MAX_SPAN; }
extern "C" int avexhip_events_chunk_windows(void) { return EV_K; }

extern "C" size_t avexhip_events_workspace_bytes(int64_t n_windows, int n_classes, int n_seq) {
    if (!ev_shape_ok(n_windows, n_classes, n_seq)) return 0;
    return ev_carve(nullptr, n_windows, n_classes, n_seq).bytes;
}

extern "C" int avexhip_events_scan(const avexhip_events_args* a, void* stream) {
    EvParams p;
    AVXH_TRY(ev_check("events_scan", a, &p));
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(EV_K);
    ev_classify_kernel<<<dim3((unsigned)p.nch * (unsigned)p.ntile), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    ev_carry_kernel<<<dim3((unsigned)p.C), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    ev_runs_kernel<<<dim3((unsigned)p.nch * (unsigned)p.C), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    ev_count_kernel<<<dim3((unsigned)p.C), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    ev_bounds_kernel<<<dim3((unsigned)p.R + 1u), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_events_emit(const avexhip_events_args* a, const avexhip_events_result* r, void* stream) {
    AVX_REQUIRE(r, "events_emit: null argument");
    AVX_REQUIRE(r->capacity >= 0 && r->capacity <= 0x7fffffffll * EV_K, "events_emit: capacity %lld outside 0 .. 2^39", (long long)r->capacity);
    AVX_REQUIRE(r->sequence && r->class_id && r->first && r->last && r->peak && r->peak_window && r->mean, "events_emit: null output");
    EvParams p;
    AVXH_TRY(ev_check("events_emit", a, &p));
    p.cap = r->capacity;
    p.o_seq = r->sequence;
    p.o_cls = r->class_id;
    p.o_first = r->first;
    p.o_last = r->last;
    p.o_peak = r->peak;
    p.o_peakw = r->peak_window;
    p.o_mean = r->mean;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(EV_K);
    ev_emit_kernel<<<dim3((unsigned)p.nch * (unsigned)p.ntile), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    ev_join_kernel<<<dim3((unsigned)p.nch * (unsigned)p.C), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    if (p.cap > 0) {
        ev_fill_kernel<<<dim3((unsigned)((p.cap + EV_K - 1) / EV_K)), block, 0, s>>>(p);
        AVX_LAUNCH_CHECK();
    }
    return AVEXHIP_OK;
}
