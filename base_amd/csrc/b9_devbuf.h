// b9_devbuf.h -- who owns the memory of a context (internal; not installed): an owning grow-only buffer, an owning list of
// uploads, the carve of one allocation into aligned parts, and the sizing rules of the work buffers and the tree buffers as
// plain functions of integers -- with the two buffer GROUPS that are keyed on more than their own size.
//
// Nothing here knows HIP.  Memory comes in through a policy `A`:
//   static int  A::alloc(void **p, void **dev_view, size_t bytes)   0, or an error code; *p null on failure.  dev_view: the block
//                                                                   as the device addresses it (mapped pinned memory: another
//                                                                   pointer; device memory: the same)
//   static void A::release(void *p)
//   static int  A::copy_in(void *dst, const void *src, size_t bytes)   (upload only)
// b9_ctx.h instantiates it with hipMalloc / hipFree and hipHostMalloc(mapped) / hipHostFree; tests/probes/devbuf_host.cpp with a
// counting allocator on the CPU.
//
// The one dialect of "too small -> free -> null -> allocate -> record the capacity" is Buf::reserve: after a failed allocation
// the pointer is null AND the capacity 0, so that the next request of any size allocates.
#pragma once
#include "../../include/base9_hip.h"

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace b9i {

// What a reservation did.  err: the policy's error code (0: fine); fresh: a new block was allocated (its contents are
// undefined: whoever needs it cleared clears it); what / bytes: the buffer and the request an error message names.
struct Reserved { int err = 0; bool fresh = false; const char *what = ""; size_t bytes = 0; };
inline Reserved named(Reserved r, const char *what) { r.what = what; return r; }

// Owning, move-only buffer of `T`.  Grows, never shrinks, never keeps its contents over a growth.
template <class T, class A>
class Buf {
public:
    Buf() = default;
    Buf(Buf &&o) noexcept { *this = std::move(o); }      // (declaring the moves deletes the copies)
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { release(); std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(cap_, o.cap_); }
        return *this;
    }
    ~Buf() { release(); }
    T *get() const { return p_; }
    T *dev() const { return dev_; }          // the same block as the device sees it
    size_t capacity() const { return cap_; } // in elements
    Reserved reserve(size_t count)
    {
        Reserved r;
        if (count <= cap_) return r;
        release();
        r.bytes = count * sizeof(T);
        void *p = nullptr, *d = nullptr;
        if ((r.err = A::alloc(&p, &d, r.bytes))) return r;
        p_ = static_cast<T *>(p); dev_ = static_cast<T *>(d); cap_ = count;
        r.fresh = true;
        return r;
    }
    void release() { if (p_) A::release(p_); p_ = dev_ = nullptr; cap_ = 0; }

private:
    T *p_ = nullptr, *dev_ = nullptr;
    size_t cap_ = 0;
};

// Owning list of device arrays that are uploaded once and read until the whole list is dropped with clear() (the pack, the
// stars, the marginalised catalogue plan).  upload: count elements of src -> a new array of the list (never a null one: an
// empty source gets one element's room); a block whose copy fails is freed at once.
template <class A> using UploadList = std::vector<Buf<char, A>>;
template <class T, class A>
Reserved upload(UploadList<A> &list, const T *src, size_t count, const T **out)
{
    Buf<char, A> b;
    Reserved r = named(b.reserve(std::max<size_t>(count, 1) * sizeof(T)), "upload");
    if (!r.err && count) r.err = A::copy_in(b.get(), src, count * sizeof(T));
    if (r.err) return r;
    *out = reinterpret_cast<const T *>(b.get());
    list.push_back(std::move(b));
    return r;
}

// One allocation cut into parts, every part on a kArenaAlign-byte boundary: take() the parts in order, allocate `total`.
constexpr size_t kArenaAlign = 256;
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t o = total; total += (bytes + kArenaAlign - 1) & ~(kArenaAlign - 1); return o; }   // -> the part's offset
};
template <class T> T *part(char *base, size_t offset) { return reinterpret_cast<T *>(base + offset); }

// b9_predict_mags' chunk of systems: mass1, mass ratio, magnitudes [chunk][nf], then wd_type, pop, stage
// (the members of a braced list are evaluated in order: each take() follows the one before it)
struct PredArena { size_t o_m1, o_q, o_mags, o_wd, o_pop, o_stage, bytes; };
inline PredArena pred_arena(size_t chunk, int nf)
{
    Carve c;
    PredArena a{c.take(8 * chunk), c.take(8 * chunk), c.take(8 * chunk * nf), c.take(4 * chunk), c.take(4 * chunk), c.take(4 * chunk), 0};
    a.bytes = c.total;
    return a;
}

// The three calls on a WD mass grid (b9_sample_wd_mass, b9_wd_moments, b9_wd_bins), one chunk of rows:
// [params][headers][isochrones][node table][per-(row, line) words [chunk][n_lines][n_col]], then the accumulators [n_lines][n_acc],
// the drawn populations [chunk][n_pop] ints, the stars' columns [n_stars] ints and the lines' edges [n_lines][n_edges].  tab_row:
// doubles of one row's node table, all populations.  A part of 0 bytes is empty: it shares its offset with the next one.
//   the draws    n_lines = n_wd, their seven outputs are the scratch (n_col = 7), n_acc = 0, n_pop = n_wd, n_edges = 0
//   the moments  n_lines = n_wd, n_col = n_acc = B9_WDM_N, n_pop = 0, n_edges = 0
//   the bins     n_lines = n_wd * n_sel, n_col = n_acc = n_bins + 3, n_pop = 0, n_edges = n_bins + 1
struct WdGridArena { size_t o_par, o_hdr, o_iso, o_tab, o_scratch, o_acc, o_pop, o_rank, o_edges, bytes; };
inline WdGridArena wd_grid_arena(size_t chunk, int n_pops, long long iso_stride, size_t tab_row, size_t n_lines, size_t n_stars, size_t n_col, size_t n_acc,
                                 size_t n_pop, size_t n_edges, size_t hdr_bytes)
{
    Carve c;
    WdGridArena a{c.take(8 * B9_NPARAM * chunk), c.take(hdr_bytes * chunk * n_pops), c.take(8 * chunk * n_pops * (size_t)iso_stride), c.take(8 * chunk * tab_row),
                  c.take(8 * chunk * n_lines * n_col), c.take(8 * n_lines * n_acc), c.take(4 * chunk * n_pop), c.take(4 * n_stars), c.take(8 * n_lines * n_edges), 0};
    a.bytes = c.total;
    return a;
}

// b9_cmd_band, one chunk of rows: [params][headers][isochrones][WD node table][value table [chunk][n_lines]], then the lines'
// pivots [n_lines], moments [n_lines][n_mom], bins [n_lines][n_bincol] and transposed edges [n_edges][n_lines].  tab_row: doubles
// of one row's WD node table, all populations.  A part of 0 bytes is empty: it shares its offset with the next one.
struct BandArena { size_t o_par, o_hdr, o_iso, o_tab, o_values, o_pivot, o_mom, o_bins, o_edges, bytes; };
inline BandArena band_arena(size_t chunk, int n_pops, long long iso_stride, size_t tab_row, size_t n_lines, size_t n_mom, size_t n_bincol, size_t n_edges,
                            size_t hdr_bytes)
{
    Carve c;
    BandArena a{c.take(8 * B9_NPARAM * chunk), c.take(hdr_bytes * chunk * n_pops), c.take(8 * chunk * n_pops * (size_t)iso_stride), c.take(8 * chunk * tab_row),
                c.take(8 * chunk * n_lines), c.take(8 * n_lines), c.take(8 * n_lines * n_mom), c.take(8 * n_lines * n_bincol), c.take(8 * n_lines * n_edges), 0};
    a.bytes = c.total;
    return a;
}

// The reductions over a saved chain (b9_star_moments, b9_mass_hist, b9_phot_resid, b9_pointwise), one chunk of rows:
// [params][headers][isochrones][node table][WD node table][per-(row, star) increments [chunk][n_stars][n_col]], then the
// accumulators [n_stars][n_acc], the chunk's per-row sums [chunk][n_rowcol], and the call's own extra parts in the order it
// lists their bytes (at most kChainExtras).  tab_row / wd_row: doubles of one row's two tables, all populations.  A part of 0
// bytes is empty: it shares its offset with the next one.
constexpr int kChainExtras = 3;
struct ChainArena { size_t o_par, o_hdr, o_iso, o_tab, o_wd, o_scratch, o_acc, o_rows, o_extra[kChainExtras], bytes; };
inline ChainArena chain_arena(size_t chunk, int n_pops, long long iso_stride, size_t tab_row, size_t wd_row, size_t n_stars, size_t n_col, size_t n_acc,
                              size_t n_rowcol, size_t hdr_bytes, const size_t (&extra_bytes)[kChainExtras])
{
    Carve c;
    ChainArena a{c.take(8 * B9_NPARAM * chunk), c.take(hdr_bytes * chunk * n_pops), c.take(8 * chunk * n_pops * (size_t)iso_stride), c.take(8 * chunk * tab_row),
                 c.take(8 * chunk * wd_row), c.take(8 * chunk * n_stars * n_col), c.take(8 * n_stars * n_acc), c.take(8 * chunk * n_rowcol), {}, 0};
    for (int k = 0; k < kChainExtras; ++k) a.o_extra[k] = c.take(extra_bytes[k]);
    a.bytes = c.total;
    return a;
}
// rows of a chunk: at most max_rows, and as few as keep the scratch [rows][n_stars][n_mom] within scratch_bytes (never less than one)
inline size_t mom_chunk_rows(size_t n_rows, size_t n_stars, size_t n_mom, size_t max_rows, size_t scratch_bytes)
{
    const size_t per_row = std::max<size_t>(1, 8 * n_stars * n_mom);
    return std::max<size_t>(1, std::min({n_rows, max_rows, scratch_bytes / per_row}));
}

// ---- sizing rules

// rows of a derived isochrone: the pack's longest one, rounded up to even; and its doubles: a mass column + nfp magnitude columns
inline int pack_mass_cap(int max_eep) { return (max_eep + 1) & ~1; }
inline long long pack_iso_stride(int mass_cap, int nfp) { return (long long)mass_cap * (nfp + 1); }

// A fused block keeps four candidate sets of W walkers in the work buffers, [2 parities][2 candidates] (StepDev), and the
// marginalised one its node tables alike.  Where candidate `cand` of parity `parity` starts: `row`, its first walker (parameter
// rows; the set's sub-set, B9IsoSet::at), and `wp`, its first (walker, population): headers, isochrones and node tables, each
// times its own length per (walker, population).
struct CandAt { size_t row, wp; };
inline CandAt cand_at(int parity, int cand, int W, int n_pops)
{
    const size_t c = (size_t)parity * 2 + cand;
    return CandAt{c * W, c * W * n_pops};
}

// The work buffers, in elements.  FOUR sets of each: the two-launch sampler (marginalised mode) ping-pongs between sets 0 and
// 1; the fused sampler step (given-mass mode) keeps two candidates for each of two step parities (StepDev).
struct WorkNeed { size_t hdr, iso, params, logpost; };
inline WorkNeed work_need(int walkers, int pops, int mass_cap, int nfp)
{
    const size_t rows = (size_t)walkers * pops;
    return WorkNeed{rows * 4, (size_t)pack_iso_stride(mass_cap, nfp) * rows * 4, (size_t)B9_NPARAM * walkers * 4, (size_t)walkers};
}

// The candidate buffers of the tree-speculative step, in elements: [2 parities][walkers][2^depth outcomes][2^depth - 1 nodes]
// candidates, each with one parameter row and -- per population -- a header and an isochrone; and the partial sums,
// [2][walkers][nodes][part_stride].
inline size_t tree_part_stride(int n_groups, int heavy_parts) { return ((size_t)n_groups * 4 + heavy_parts + 1) & ~(size_t)1; }
struct TreeNeed { size_t n_cand, hdr, iso, par, partial; };
inline TreeNeed tree_need(int walkers, int pops, int depth, long long iso_stride, int n_groups, int heavy_parts)
{
    const size_t NN = ((size_t)1 << depth) - 1, NO = (size_t)1 << depth, n_cand = (size_t)2 * walkers * NO * NN;
    return TreeNeed{n_cand, n_cand * pops, (size_t)iso_stride * n_cand * pops, (size_t)B9_NPARAM * n_cand,
                    (size_t)2 * walkers * NN * tree_part_stride(n_groups, heavy_parts)};
}

// ---- the two groups

// The work buffers.  They are indexed with the group's own key (buffer_set: set s of the parameters starts at s * cap_walkers
// rows), so the four are reallocated together whenever the key changes: more walkers or populations than ever before, or a
// pack with another isochrone length or filter count (the rows depend on BOTH: a pack reloaded with the same EEP count but
// more filters needs wider rows).
template <class Hdr, class A>
struct WorkBufs {
    int cap_walkers = 0, cap_pops = 0, mass_cap = 0;
    long long iso_stride = 0;
    Buf<Hdr, A> hdr;
    Buf<double, A> iso, params, logpost;

    Reserved ensure(int walkers, int pops, int max_eep, int nfp)
    {
        const int want_cap = pack_mass_cap(max_eep);
        if (walkers <= cap_walkers && pops <= cap_pops && mass_cap == want_cap && iso_stride == pack_iso_stride(want_cap, nfp)) return Reserved{};
        const int cw = std::max(walkers, cap_walkers), cp = std::max(pops, cap_pops);
        const WorkNeed need = work_need(cw, cp, want_cap, nfp);
        cap_walkers = cap_pops = 0;          // the key says "nothing fits" until all four exist: a failure makes the next call start over
        mass_cap = want_cap; iso_stride = pack_iso_stride(want_cap, nfp);
        hdr.release(); iso.release(); params.release(); logpost.release();
        Reserved r;
        if ((r = hdr.reserve(need.hdr)).err) return named(r, "work buffers: isochrone headers");
        if ((r = iso.reserve(need.iso)).err) return named(r, "work buffers: isochrones");
        if ((r = params.reserve(need.params)).err) return named(r, "work buffers: parameter rows");
        if ((r = logpost.reserve(need.logpost)).err) return named(r, "work buffers: log-posteriors");
        cap_walkers = cw; cap_pops = cp;
        return r;
    }
};

// The tree step's buffers.  Each reserves its OWN need (the parameter rows do not scale with the populations, the other two
// candidate buffers do); a pack with another row length starts the three candidate buffers afresh.  hdr_fresh /
// partial_fresh: that buffer is a new block, which the caller clears.
template <class Hdr, class A>
struct TreeBufs {
    long long iso_stride = 0;
    Buf<Hdr, A> hdr;
    Buf<double, A> iso, par, partial;
    bool hdr_fresh = false, partial_fresh = false;

    Reserved ensure(int walkers, int pops, int depth, long long stride, int n_groups, int heavy_parts)
    {
        hdr_fresh = partial_fresh = false;
        if (stride != iso_stride) { hdr.release(); iso.release(); par.release(); iso_stride = stride; }
        const TreeNeed need = tree_need(walkers, pops, depth, stride, n_groups, heavy_parts);
        Reserved r;
        if ((r = hdr.reserve(need.hdr)).err) return named(r, "tree buffers: isochrone headers");
        hdr_fresh = r.fresh;
        if ((r = iso.reserve(need.iso)).err) return named(r, "tree buffers: isochrones");
        if ((r = par.reserve(need.par)).err) return named(r, "tree buffers: parameter rows");
        if ((r = partial.reserve(need.partial)).err) return named(r, "tree buffers: partial sums");
        partial_fresh = r.fresh;
        return r;
    }
};

}  // namespace b9i
