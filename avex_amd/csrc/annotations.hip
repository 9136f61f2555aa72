// Scoring detections against annotations (ABI 22): sample overlap of every window with every class, and the matching of predicted events
// (events.hip's columns, where they lie) with reference events.  The reference project has no such step.
//
// Reference events are per (recording, class) SEGMENT the annotations merged where they overlap or touch: disjoint, ordered by lo and so
// by hi as well.  Every decision is integer arithmetic on sample counts, or one fp64 multiply and compare (the library is built with
// -ffp-contract=off, and there is no add beside the multiply to contract).  No kernel here holds an atomic.
//
//   an_overlap_kernel   one thread per (window, class), classes fastest: the events with hi > span_lo and lo < span_hi by two binary
//                       searches inside the segment, their summed length from the prefix, the two edge events clipped.
//   an_count_kernel     one thread per prediction: its span [cell_lo[first], cell_hi[last]), its segment, the events it overlaps (the same
//                       two searches, kept in the workspace), the compatible ones counted; the row checked against the row before it.
//   an_fill_kernel      -1 into both match arrays.
//   an_emit_kernel      one thread per prediction writes its pairs (i, j) at pair_offsets[i] ..: the pairs of all predictions in (i, j) order.
//   an_reduce_kernel    the walk "compatible -> match both and advance both, else advance the one that ends first" takes a pair iff neither
//   an_carry_kernel     of its two events is matched yet, in (i, j) order.  That is a scan of functions on two bits of state (prediction
//   an_apply_kernel     matched, event matched): a pair with a new prediction clears the first bit, with a new event the second, and is
//                       taken when both are clear, which sets both.  A function on four states is a byte, composition four look-ups.
//                       Chunks of AN_K = 256 pairs are reduced to one function each, one workgroup carries the state over the chunk
//                       functions (ev_carry_kernel's shape), and the chunks are applied again with the state that enters them.  Pair
//                       numbers are global, so a segment boundary (a new prediction AND a new event) resets the state by itself.
// A thread's sequential work is bounded by the reference events its own prediction overlaps (in all at most n_pred + n_ref pairs for
// ordered input), never by the size of a segment.  Unordered or overlapping predictions cannot leave an array: searches are clamped to
// [0, n_ref), pairs past the buffer are dropped, and such rows are flagged in errors[].
#include "block_prims.h"
#include "common.h"

namespace {

constexpr int AN_K = AVEXHIP_ANNOT_CHUNK_PAIRS;   // pairs of one chunk = threads of a workgroup
constexpr int AN_WAVES = AN_K / 64;
constexpr int64_t AN_MAX = 0x7fffffffll;
constexpr unsigned AN_ID = 0xE4u;                 // the identity on the states 0 .. 3, two bits each

struct AnWs {
    int32_t* j0;              // [P]  first event the prediction overlaps
    int32_t* j1;              // [P]  one past the last
    int32_t* pi;              // [P + A]  pairs: prediction
    int32_t* pj;              //          reference event
    unsigned char* summ;      // [chunks]  the chunk's function
    unsigned char* carry;     // [chunks]  state entering the chunk
    size_t bytes;
};

static inline int64_t an_chunks(int64_t n_pred, int64_t n_ref) { return (n_pred + n_ref + AN_K - 1) / AN_K; }

static AnWs an_carve(void* ws, int64_t n_pred, int64_t n_ref) {
    const size_t P = (size_t)n_pred, cap = (size_t)(n_pred + n_ref), nch = (size_t)an_chunks(n_pred, n_ref);
    const size_t step = 16;      // bytes: every array starts 16-byte aligned
    AnWs w;
    char* p = (char*)ws;
    w.j0 = take<int32_t>(p, P, step);
    w.j1 = take<int32_t>(p, P, step);
    w.pi = take<int32_t>(p, cap, step);
    w.pj = take<int32_t>(p, cap, step);
    w.summ = take<unsigned char>(p, nch, step);
    w.carry = take<unsigned char>(p, nch, step);
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

static bool an_shape_ok(int64_t n_pred, int64_t n_ref, int64_t n_seg) {
    return n_pred >= 1 && n_ref >= 1 && n_seg >= 1 && n_pred <= AN_MAX && n_ref <= AN_MAX && n_seg <= AN_MAX && n_pred + n_ref <= AN_MAX - AN_K;
}

struct AnParams {
    const int32_t* seq;
    const int32_t* cls;
    const int32_t* first;
    const int32_t* last;
    int P, A, N, R, C;
    int nch;
    const int64_t* cell_lo;
    const int64_t* cell_hi;
    const int64_t* seg;
    const int64_t* rlo;
    const int64_t* rhi;
    double iou;
    AnWs w;
    int64_t* counts;
    int32_t* errors;
    const int64_t* pair_off;
    int32_t* mop;
    int32_t* mor;
};

// the events [a, b) of a segment, clamped into the table: a device copy of the offsets that differs from the checked one cannot leave it
static __device__ __forceinline__ void an_segment(const int64_t* __restrict__ seg, int64_t s, int64_t A, int64_t& a, int64_t& b) {
    a = seg[s];
    b = seg[s + 1];
    a = a < 0 ? 0 : (a > A ? A : a);
    b = b < a ? a : (b > A ? A : b);
}
// the first j in [a, b) with hi[j] > x (b if none)
static __device__ __forceinline__ int64_t an_first_hi_above(const int64_t* __restrict__ hi, int64_t a, int64_t b, int64_t x) {
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (hi[m] > x) b = m; else a = m + 1;
    }
    return a;
}
// the first j in [a, b) with lo[j] >= x (b if none)
static __device__ __forceinline__ int64_t an_first_lo_from(const int64_t* __restrict__ lo, int64_t a, int64_t b, int64_t x) {
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (lo[m] >= x) b = m; else a = m + 1;
    }
    return a;
}

__global__ __launch_bounds__(256) void an_overlap_kernel(const int64_t* __restrict__ span_lo, const int64_t* __restrict__ span_hi, const int32_t* __restrict__ win_rec,
                                                         int64_t n_win, int n_rec, int C, const int64_t* __restrict__ seg, const int64_t* __restrict__ rlo,
                                                         const int64_t* __restrict__ rhi, const int64_t* __restrict__ prefix, int64_t A, int32_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_win * (int64_t)C) return;
    const int64_t w = idx / C;
    const int c = (int)(idx - w * C);
    const int r = win_rec[w];
    const int64_t lo = span_lo[w], hi = span_hi[w];
    int64_t cov = 0;
    if (r >= 0 && r < n_rec && hi > lo) {
        int64_t a, b;
        an_segment(seg, (int64_t)r * C + c, A, a, b);
        const int64_t j0 = an_first_hi_above(rhi, a, b, lo), j1 = an_first_lo_from(rlo, j0, b, hi);
        if (j1 > j0) {
            cov = prefix[j1] - prefix[j0];
            const int64_t head = lo - rlo[j0], tail = rhi[j1 - 1] - hi;      // what the first and the last event hold outside the span
            cov -= head > 0 ? head : 0;
            cov -= tail > 0 ? tail : 0;
        }
    }
    out[idx] = (int32_t)(cov < 0 ? 0 : (cov > AN_MAX ? AN_MAX : cov));
}

// row i of the prediction columns: 0 a filler row, 1 a prediction (its segment and span set), -1 a row that is neither
static __device__ __forceinline__ int an_pred(const AnParams& p, int i, int64_t& s, int64_t& lo, int64_t& hi) {
    const int f = p.first[i];
    if (f < 0) return 0;
    const int l = p.last[i], r = p.seq[i], c = p.cls[i];
    if (l < f || l >= p.N || r < 0 || r >= p.R || c < 0 || c >= p.C) return -1;
    s = (int64_t)r * p.C + c;
    lo = p.cell_lo[f];
    hi = p.cell_hi[l];
    return 1;
}

static __device__ __forceinline__ bool an_compatible(int64_t plo, int64_t phi, int64_t rlo, int64_t rhi, double iou) {
    const int64_t inter = (phi < rhi ? phi : rhi) - (plo > rlo ? plo : rlo);
    const int64_t uni = (phi > rhi ? phi : rhi) - (plo < rlo ? plo : rlo);       // the two spans meet: their union is their hull
    return inter > 0 && (double)inter >= iou * (double)uni;
}

__global__ __launch_bounds__(AN_K) void an_count_kernel(AnParams p) {
    const int64_t i64 = (int64_t)blockIdx.x * AN_K + threadIdx.x;
    if (i64 >= p.P) return;
    const int i = (int)i64;
    int64_t s = 0, lo = 0, hi = 0;
    const int st = an_pred(p, i, s, lo, hi);
    int err = st < 0 ? 1 : 0;
    if (st > 0 && i > 0) {
        int64_t sp = 0, lop = 0, hip = 0;
        const int stp = an_pred(p, i - 1, sp, lop, hip);
        if (stp == 0 || (stp > 0 && (sp > s || (sp == s && hip > lo)))) err = 1;      // behind a filler row, or not after the row before it
    }
    int64_t j0 = 0, j1 = 0, cnt = 0;
    if (st > 0 && hi > lo) {
        int64_t a, b;
        an_segment(p.seg, s, p.A, a, b);
        j0 = an_first_hi_above(p.rhi, a, b, lo);
        j1 = an_first_lo_from(p.rlo, j0, b, hi);
        for (int64_t j = j0; j < j1; ++j) cnt += an_compatible(lo, hi, p.rlo[j], p.rhi[j], p.iou) ? 1 : 0;
    }
    p.w.j0[i] = (int32_t)j0;
    p.w.j1[i] = (int32_t)j1;
    p.counts[i] = cnt;
    p.errors[i] = err;
}

__global__ __launch_bounds__(AN_K) void an_fill_kernel(int32_t* __restrict__ mop, int P, int32_t* __restrict__ mor, int A) {
    const int64_t i = (int64_t)blockIdx.x * AN_K + threadIdx.x;
    if (i < P) mop[i] = -1;
    if (i < A) mor[i] = -1;
}

__global__ __launch_bounds__(AN_K) void an_emit_kernel(AnParams p) {
    const int64_t i64 = (int64_t)blockIdx.x * AN_K + threadIdx.x;
    if (i64 >= p.P) return;
    const int i = (int)i64;
    const int j0 = p.w.j0[i], j1 = p.w.j1[i];
    if (j1 <= j0) return;                              // a filler row, a malformed one, an empty span, or nothing under the span
    int64_t s, lo, hi;
    if (an_pred(p, i, s, lo, hi) <= 0) return;
    const int64_t cap = (int64_t)p.P + p.A;
    int64_t at = p.pair_off[i];
    for (int j = j0; j < j1; ++j) {
        if (!an_compatible(lo, hi, p.rlo[j], p.rhi[j], p.iou)) continue;
        if (at >= 0 && at < cap) {
            p.w.pi[at] = i;
            p.w.pj[at] = j;
        }
        ++at;
    }
}

// f then g: the operator of the block scans below (associative, not commutative; AN_ID its identity)
struct AnCompose {
    __device__ __forceinline__ unsigned operator()(unsigned f, unsigned g) const {
        unsigned h = 0u;
#pragma unroll
        for (int s = 0; s < 4; ++s) h |= ((g >> (2u * ((f >> (2 * s)) & 3u))) & 3u) << (2 * s);
        return h;
    }
};
static __device__ __forceinline__ int an_apply(unsigned f, int s) { return (int)((f >> (2 * s)) & 3u); }

// the function of pair k (identity past the last pair): bit 0 of the state = the prediction is matched, bit 1 = the event is
static __device__ __forceinline__ unsigned an_pair_fn(const AnParams& p, int64_t k, int64_t total, bool& new_pred, bool& new_ref) {
    new_pred = new_ref = false;
    if (k >= total) return AN_ID;
    new_pred = k == 0 || p.w.pi[k] != p.w.pi[k - 1];
    new_ref = k == 0 || p.w.pj[k] != p.w.pj[k - 1];
    unsigned f = 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int t = s & ~((new_pred ? 1 : 0) | (new_ref ? 2 : 0));
        f |= (unsigned)(t == 0 ? 3 : t) << (2 * s);
    }
    return f;
}

static __device__ __forceinline__ int64_t an_total(const AnParams& p) {
    const int64_t cap = (int64_t)p.P + p.A, t = p.pair_off[p.P];
    return t < 0 ? 0 : (t > cap ? cap : t);
}

// The scans below run the workgroup's 256 functions in thread order (block_scan, block_prims.h): `before` is the composition of the
// threads BELOW this one, `all` of all of them.
__global__ __launch_bounds__(AN_K) void an_reduce_kernel(AnParams p) {
    __shared__ unsigned wt[AN_WAVES];
    const int64_t k = (int64_t)blockIdx.x * AN_K + threadIdx.x;
    bool np, nr;
    const unsigned f = an_pair_fn(p, k, an_total(p), np, nr);
    unsigned before, all;
    block_scan<AN_WAVES>(f, AN_ID, AnCompose(), wt, &before, &all);
    if (threadIdx.x == 0) p.w.summ[blockIdx.x] = (unsigned char)all;
}

// One workgroup; thread t owns chunk base + t of the pass.
__global__ __launch_bounds__(AN_K) void an_carry_kernel(AnParams p) {
    __shared__ unsigned wt[AN_WAVES];
    int state = 0;                                    // entering chunk `base`: nothing matched
    for (int base = 0; base < p.nch; base += AN_K) {
        const int k = base + threadIdx.x;
        const unsigned f = k < p.nch ? (unsigned)p.w.summ[k] : AN_ID;
        unsigned before, all;
        block_scan<AN_WAVES>(f, AN_ID, AnCompose(), wt, &before, &all);
        if (k < p.nch) p.w.carry[k] = (unsigned char)an_apply(before, state);
        state = an_apply(all, state);
    }
}

__global__ __launch_bounds__(AN_K) void an_apply_kernel(AnParams p) {
    __shared__ unsigned wt[AN_WAVES];
    const int64_t k = (int64_t)blockIdx.x * AN_K + threadIdx.x;
    const int64_t total = an_total(p);
    bool np, nr;
    const unsigned f = an_pair_fn(p, k, total, np, nr);
    unsigned before, all;
    block_scan<AN_WAVES>(f, AN_ID, AnCompose(), wt, &before, &all);
    if (k >= total) return;
    const int s = an_apply(before, (int)p.w.carry[blockIdx.x]) & ~((np ? 1 : 0) | (nr ? 2 : 0));
    if (s != 0) return;                               // one of the two is matched already
    const int i = p.w.pi[k], j = p.w.pj[k];
    if (i >= 0 && i < p.P && j >= 0 && j < p.A) {     // (always, for pairs this call wrote)
        p.mop[i] = j;
        p.mor[j] = i;
    }
}

static int an_offsets_check(const char* what, const int64_t* off, int64_t n_seg, int64_t n_ref) {
    AVX_REQUIRE(off[0] == 0, "%s: seg_offsets[0] = %lld, not 0", what, (long long)off[0]);
    for (int64_t s = 0; s < n_seg; ++s)
        AVX_REQUIRE(off[s + 1] >= off[s], "%s: seg_offsets[%lld] = %lld < seg_offsets[%lld] = %lld", what, (long long)(s + 1), (long long)off[s + 1], (long long)s,
                    (long long)off[s]);
    AVX_REQUIRE(off[n_seg] == n_ref, "%s: seg_offsets[%lld] = %lld, not n_ref %lld", what, (long long)n_seg, (long long)off[n_seg], (long long)n_ref);
    return AVEXHIP_OK;
}

static int an_check(const char* what, const avexhip_annot_match_args* a, AnParams* p) {
    AVX_REQUIRE(a && a->sequence && a->class_id && a->first && a->last && a->cell_lo && a->cell_hi && a->seg_offsets_host && a->seg_offsets_dev && a->ref_lo &&
                    a->ref_hi && a->workspace && a->counts && a->errors,
                "%s: null argument", what);
    AVX_REQUIRE((((uintptr_t)a->sequence | (uintptr_t)a->class_id | (uintptr_t)a->first | (uintptr_t)a->last | (uintptr_t)a->errors) & 3) == 0 &&
                    (((uintptr_t)a->cell_lo | (uintptr_t)a->cell_hi | (uintptr_t)a->seg_offsets_dev | (uintptr_t)a->ref_lo | (uintptr_t)a->ref_hi | (uintptr_t)a->counts) & 7) == 0 &&
                    ((uintptr_t)a->workspace & 15) == 0,
                "%s: int32 arrays must be 4-byte aligned, int64 arrays 8-byte aligned, the workspace 16-byte aligned", what);
    AVX_REQUIRE(a->n_rec >= 1 && a->n_classes >= 1 && (int64_t)a->n_rec * a->n_classes <= AN_MAX, "%s: n_rec=%d n_classes=%d", what, a->n_rec, a->n_classes);
    AVX_REQUIRE(a->n_windows >= 1 && a->n_windows <= AN_MAX, "%s: n_windows=%lld outside 1 .. 2^31 - 1", what, (long long)a->n_windows);
    const int64_t n_seg = (int64_t)a->n_rec * a->n_classes;
    AVX_REQUIRE(an_shape_ok(a->n_pred, a->n_ref, n_seg), "%s: bad shape (n_pred %lld, n_ref %lld: each >= 1, together below 2^31 - 256)", what, (long long)a->n_pred,
                (long long)a->n_ref);
    AVX_REQUIRE(a->iou >= AVEXHIP_ANNOT_MIN_IOU && a->iou <= 1.0, "%s: iou=%g outside %g .. 1", what, a->iou, (double)AVEXHIP_ANNOT_MIN_IOU);      // (a NaN fails both)
    AVXH_TRY(an_offsets_check(what, a->seg_offsets_host, n_seg, a->n_ref));
    const AnWs w = an_carve(a->workspace, a->n_pred, a->n_ref);
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("%s: workspace %zu B < %zu B", what, a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    memset(p, 0, sizeof(*p));
    p->seq = a->sequence;
    p->cls = a->class_id;
    p->first = a->first;
    p->last = a->last;
    p->P = (int)a->n_pred;
    p->A = (int)a->n_ref;
    p->N = (int)a->n_windows;
    p->R = a->n_rec;
    p->C = a->n_classes;
    p->nch = (int)an_chunks(a->n_pred, a->n_ref);
    p->cell_lo = a->cell_lo;
    p->cell_hi = a->cell_hi;
    p->seg = a->seg_offsets_dev;
    p->rlo = a->ref_lo;
    p->rhi = a->ref_hi;
    p->iou = a->iou;
    p->w = w;
    p->counts = a->counts;
    p->errors = a->errors;
    return AVEXHIP_OK;
}

}  // namespace

extern "C" int avexhip_annot_chunk_pairs(void) { return AN_K; }

extern "C" size_t avexhip_annot_workspace_bytes(int64_t n_pred, int64_t n_ref, int64_t n_segments) {
    if (!an_shape_ok(n_pred, n_ref, n_segments)) return 0;
    return an_carve(nullptr, n_pred, n_ref).bytes;    // the segments take no room: their offsets are the caller's
}

extern "C" int avexhip_annot_overlap(const int64_t* span_lo_dev, const int64_t* span_hi_dev, const int32_t* win_rec_host, const int32_t* win_rec_dev,
                                     int64_t n_win, int n_rec, int n_classes, const int64_t* seg_offsets_host, const int64_t* seg_offsets_dev,
                                     const int64_t* ref_lo_dev, const int64_t* ref_hi_dev, const int64_t* ref_prefix_dev, int64_t n_ref, int32_t* out_dev,
                                     void* stream) {
    AVX_REQUIRE(span_lo_dev && span_hi_dev && win_rec_host && win_rec_dev && seg_offsets_host && seg_offsets_dev && ref_lo_dev && ref_hi_dev && ref_prefix_dev && out_dev,
                "annot_overlap: null argument");
    AVX_REQUIRE((((uintptr_t)span_lo_dev | (uintptr_t)span_hi_dev | (uintptr_t)seg_offsets_dev | (uintptr_t)ref_lo_dev | (uintptr_t)ref_hi_dev | (uintptr_t)ref_prefix_dev) & 7) == 0 &&
                    (((uintptr_t)win_rec_dev | (uintptr_t)out_dev) & 3) == 0,
                "annot_overlap: int64 arrays must be 8-byte aligned, int32 arrays 4-byte aligned");
    AVX_REQUIRE(n_rec >= 1 && n_classes >= 1 && (int64_t)n_rec * n_classes <= AN_MAX, "annot_overlap: n_rec=%d n_classes=%d", n_rec, n_classes);
    AVX_REQUIRE(n_win >= 1 && n_win <= AN_MAX && n_win <= AN_MAX * 256 / n_classes, "annot_overlap: n_win=%lld with %d classes: more entries than one launch takes",
                (long long)n_win, n_classes);
    AVX_REQUIRE(n_ref >= 1 && n_ref <= AN_MAX, "annot_overlap: n_ref=%lld outside 1 .. 2^31 - 1", (long long)n_ref);
    AVXH_TRY(an_offsets_check("annot_overlap", seg_offsets_host, (int64_t)n_rec * n_classes, n_ref));
    for (int64_t w = 0; w < n_win; ++w)
        AVX_REQUIRE(win_rec_host[w] >= 0 && win_rec_host[w] < n_rec, "annot_overlap: window %lld: recording %d outside the %d", (long long)w, win_rec_host[w], n_rec);
    const int64_t blocks = (n_win * n_classes + 255) / 256;
    hipLaunchKernelGGL(an_overlap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, span_lo_dev, span_hi_dev, win_rec_dev, n_win, n_rec, n_classes,
                       seg_offsets_dev, ref_lo_dev, ref_hi_dev, ref_prefix_dev, n_ref, out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_annot_count(const avexhip_annot_match_args* args, void* stream) {
    AnParams p;
    AVXH_TRY(an_check("annot_count", args, &p));
    an_count_kernel<<<dim3((unsigned)((p.P + AN_K - 1) / AN_K)), dim3(AN_K), 0, (hipStream_t)stream>>>(p);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_annot_match(const avexhip_annot_match_args* args, const int64_t* pair_offsets_dev, int32_t* match_of_pred_dev, int32_t* match_of_ref_dev,
                                   void* stream) {
    AVX_REQUIRE(pair_offsets_dev && match_of_pred_dev && match_of_ref_dev, "annot_match: null argument");
    AVX_REQUIRE(((uintptr_t)pair_offsets_dev & 7) == 0 && (((uintptr_t)match_of_pred_dev | (uintptr_t)match_of_ref_dev) & 3) == 0,
                "annot_match: pair_offsets_dev must be 8-byte aligned, the match arrays 4-byte aligned");
    AnParams p;
    AVXH_TRY(an_check("annot_match", args, &p));
    p.pair_off = pair_offsets_dev;
    p.mop = match_of_pred_dev;
    p.mor = match_of_ref_dev;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(AN_K);
    const int big = p.P > p.A ? p.P : p.A;
    an_fill_kernel<<<dim3((unsigned)((big + AN_K - 1) / AN_K)), block, 0, s>>>(p.mop, p.P, p.mor, p.A);
    AVX_LAUNCH_CHECK();
    an_emit_kernel<<<dim3((unsigned)((p.P + AN_K - 1) / AN_K)), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    an_reduce_kernel<<<dim3((unsigned)p.nch), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    an_carry_kernel<<<dim3(1), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    an_apply_kernel<<<dim3((unsigned)p.nch), block, 0, s>>>(p);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
