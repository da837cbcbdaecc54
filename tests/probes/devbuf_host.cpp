// devbuf_host.cpp -- the shipped base_amd/csrc/b9_devbuf.h, unchanged, on the CPU: a counting allocator that can be told to
// fail its N-th call stands in for the HIP policies.  A stand-alone program (tests/test_devbuf_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process); exits non-zero at the first violated line.
#include "../../base_amd/csrc/b9_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

using namespace b9i;

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: violated: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Counting {
    static int n_alloc, n_free, fail_at, n_copy, fail_copy_at;     // fail_at = N: the N-th alloc since reset() fails (0: none)
    static std::set<void *> live;
    static void reset(int fail = 0, int fail_copy = 0) { n_alloc = n_free = n_copy = 0; fail_at = fail; fail_copy_at = fail_copy; }
    static int alloc(void **p, void **dev, size_t bytes)
    {
        *p = *dev = nullptr;
        if (++n_alloc == fail_at) return 2;
        *p = std::malloc(bytes ? bytes : 1);
        CHECK(*p);
        std::memset(*p, 0xA5, bytes);        // (the whole request is writable: ASan sees an undersized block)
        *dev = *p;
        live.insert(*p);
        return 0;
    }
    static void release(void *p)
    {
        CHECK(live.erase(p) == 1);           // a block of ours, freed once
        ++n_free;
        std::free(p);
    }
    static int copy_in(void *dst, const void *src, size_t bytes)
    {
        if (++n_copy == fail_copy_at) return 3;
        std::memcpy(dst, src, bytes);
        return 0;
    }
};
int Counting::n_alloc = 0, Counting::n_free = 0, Counting::fail_at = 0, Counting::n_copy = 0, Counting::fail_copy_at = 0;
std::set<void *> Counting::live;

struct Hdr { double a, b, c; int n, first, valid, pad; };       // stands in for IsoHdr: only its size matters here

// Runs `scenario` once without a failure, then once per allocation it made with that allocation failing: nothing may be
// live when it returns, wherever the failure falls.
template <class F>
int at_every_failure_point(F scenario)
{
    Counting::reset();
    scenario();
    CHECK(Counting::live.empty());
    const int n = Counting::n_alloc;
    CHECK(n > 0);
    for (int k = 1; k <= n; ++k) {
        Counting::reset(k);
        scenario();
        CHECK(Counting::live.empty());
    }
    return n;
}

// ---- Buf
void buf_scenario()
{
    Buf<double, Counting> b;
    CHECK(!b.get() && b.capacity() == 0);
    Reserved r = b.reserve(0);
    CHECK(!r.err && !r.fresh && !b.get());                    // nothing asked, nothing allocated
    const int a0 = Counting::n_alloc, f0 = Counting::n_free;
    r = b.reserve(100);
    if (!r.err) {
        CHECK(r.fresh && b.get() && b.dev() == b.get() && b.capacity() == 100 && r.bytes == 800);
        CHECK(Counting::n_alloc == a0 + 1 && Counting::n_free == f0);
        r = b.reserve(40);                                    // never shrinks
        CHECK(!r.err && !r.fresh && b.capacity() == 100 && Counting::n_alloc == a0 + 1);
    } else {
        CHECK(!r.fresh && !b.get() && !b.dev() && b.capacity() == 0);
    }
    const int a1 = Counting::n_alloc, f1 = Counting::n_free;
    const bool had = b.get() != nullptr;
    r = b.reserve(300);                                       // growth: the old block goes exactly once
    CHECK(Counting::n_alloc == a1 + 1 && Counting::n_free == f1 + (had ? 1 : 0));
    if (r.err) {
        CHECK(!b.get() && b.capacity() == 0);                 // null AND 0 ...
        const int a2 = Counting::n_alloc;
        r = b.reserve(7);                                     // ... so the next request of ANY size allocates
        CHECK(Counting::n_alloc == a2 + 1);
        CHECK(r.err || (r.fresh && b.get() && b.capacity() == 7));
    } else {
        CHECK(r.fresh && b.capacity() == 300);
    }
    // moves: the moved-from buffer frees nothing
    const int f2 = Counting::n_free;
    double *const p = b.get();
    const size_t cap = b.capacity();
    {
        Buf<double, Counting> c(std::move(b));
        CHECK(!b.get() && b.capacity() == 0 && c.get() == p && c.capacity() == cap);
        Buf<double, Counting> d;
        (void)d.reserve(5);
        const int f3 = Counting::n_free;
        const bool d_had = d.get() != nullptr;
        d = std::move(c);                                     // d's own block goes, c's moves in
        CHECK(Counting::n_free == f3 + (d_had ? 1 : 0) && !c.get() && d.get() == p);
    }                                                         // c (empty) and d (owner) die here
    CHECK(Counting::n_free >= f2 + (p ? 1 : 0));
    const int f4 = Counting::n_free;
    b.release();                                              // moved-from: nothing to free
    CHECK(Counting::n_free == f4);
}

// ---- UploadList
void upload_scenario()
{
    UploadList<Counting> u;
    const int src[5] = {1, 2, 3, 4, 5};
    const int *d1 = nullptr, *d0 = nullptr;
    Reserved r = upload(u, src, 5, &d1);
    if (!r.err) { CHECK(d1 && u.size() == 1 && std::memcmp(d1, src, sizeof src) == 0 && r.bytes == sizeof src); }
    else CHECK(!d1 && u.size() == 0);
    const size_t n1 = u.size();
    r = upload(u, src, 0, &d0);                                // an empty source still gets a (non-null) array
    if (!r.err) CHECK(d0 && u.size() == n1 + 1 && r.bytes == sizeof(int));
    const size_t n2 = u.size();
    u.clear();
    CHECK(u.size() == 0 && Counting::n_free >= (int)n2);
    const double x[3] = {1.0, 2.0, 3.0};
    const double *dx = nullptr;
    (void)upload(u, x, 3, &dx);                                // left to the destructor
}

void upload_copy_failure()
{
    Counting::reset(0, 2);                                    // the second copy fails
    {
        UploadList<Counting> u;
        const int src[3] = {7, 8, 9};
        const int *a = nullptr, *b = nullptr;
        CHECK(!upload(u, src, 3, &a).err && a && u.size() == 1);
        const int f0 = Counting::n_free;
        const Reserved r = upload(u, src, 3, &b);
        CHECK(r.err == 3 && !b && u.size() == 1);
        CHECK(Counting::n_alloc == 2 && Counting::n_free == f0 + 1 && Counting::live.size() == 1);   // its block is freed at once
    }
    CHECK(Counting::live.empty());
}

// ---- the work-buffer group
struct WorkStep { int walkers, pops, max_eep, nfp; };
// first use -> more walkers -> second population -> a pack with more filters at the same EEP count -> fewer walkers
const WorkStep kWorkSteps[] = {{4, 1, 119, 4}, {8, 1, 119, 4}, {8, 2, 119, 4}, {8, 2, 119, 8}, {2, 2, 119, 8}};

void check_work(const WorkBufs<Hdr, Counting> &w, const WorkStep &s)
{
    CHECK(w.mass_cap == pack_mass_cap(s.max_eep) && w.iso_stride == pack_iso_stride(w.mass_cap, s.nfp));
    CHECK(w.cap_walkers >= s.walkers && w.cap_pops >= s.pops);
    // what the call needs, and what buffer_set's indexing with the key itself needs
    for (const WorkNeed &n : {work_need(s.walkers, s.pops, w.mass_cap, s.nfp), work_need(w.cap_walkers, w.cap_pops, w.mass_cap, s.nfp)}) {
        CHECK(w.hdr.capacity() >= n.hdr && w.iso.capacity() >= n.iso && w.params.capacity() >= n.params && w.logpost.capacity() >= n.logpost);
    }
}

void work_scenario()
{
    WorkBufs<Hdr, Counting> w;
    for (const WorkStep &s : kWorkSteps) {
        Reserved r = w.ensure(s.walkers, s.pops, s.max_eep, s.nfp);
        if (r.err) {
            CHECK(w.cap_walkers == 0 && w.cap_pops == 0 && r.what[0] && r.bytes > 0);     // the key says "start over"
            const int a0 = Counting::n_alloc;
            r = w.ensure(s.walkers, s.pops, s.max_eep, s.nfp);                             // (the injected failure is spent)
            CHECK(!r.err && Counting::n_alloc == a0 + 4);                                  // ... and the next call reallocates all four
        }
        check_work(w, s);
    }
    const int a1 = Counting::n_alloc;
    CHECK(!w.ensure(2, 2, 119, 8).err && Counting::n_alloc == a1);                         // satisfied: nothing happens
}

void work_sequence_allocations()
{
    // without failures: four allocations at each of the first four steps (each changes the key), none at the fifth
    Counting::reset();
    {
        WorkBufs<Hdr, Counting> w;
        int want = 0;
        for (const WorkStep &s : kWorkSteps) {
            CHECK(!w.ensure(s.walkers, s.pops, s.max_eep, s.nfp).err);
            if (&s != &kWorkSteps[4]) want += 4;
            CHECK(Counting::n_alloc == want && (int)Counting::live.size() == 4);
            check_work(w, s);
        }
        // a regrowth (more walkers) with a failure at each of its four allocations in turn: the call after it reallocates all four
        for (int k = 1; k <= 4; ++k) {
            const WorkStep s{16 * k, 2, 119, 8};
            Counting::reset(k);
            const Reserved r = w.ensure(s.walkers, s.pops, s.max_eep, s.nfp);
            CHECK(r.err == 2 && Counting::n_alloc == k && w.cap_walkers == 0 && w.cap_pops == 0);
            Counting::reset();
            // (even a SMALLER request than any before: the reloaded-pack case, where walkers <= the old cap_walkers)
            const WorkStep t{2, 1, 119, 8};
            CHECK(!w.ensure(t.walkers, t.pops, t.max_eep, t.nfp).err && Counting::n_alloc == 4);
            check_work(w, t);
            CHECK(!w.ensure(s.walkers, s.pops, s.max_eep, s.nfp).err);
            check_work(w, s);
        }
    }
    CHECK(Counting::live.empty());
}

// ---- the tree group
struct TreeStep { int walkers, pops, depth; };
const TreeStep kTreeSteps[] = {{2, 2, 3}, {4, 1, 3}, {2, 2, 2}, {4, 1, 3}};
constexpr long long kTreeStride = 20 * 5;
constexpr int kTreeGroups = 3, kTreeHeavy = 4;

void check_tree(const TreeBufs<Hdr, Counting> &t, const TreeStep &s)
{
    const TreeNeed n = tree_need(s.walkers, s.pops, s.depth, kTreeStride, kTreeGroups, kTreeHeavy);
    CHECK(n.n_cand == (size_t)2 * s.walkers * (1u << s.depth) * ((1u << s.depth) - 1));
    CHECK(t.par.capacity() >= (size_t)B9_NPARAM * n.n_cand);
    CHECK(t.hdr.capacity() >= n.hdr && t.iso.capacity() >= n.iso && t.partial.capacity() >= n.partial);
}

void tree_scenario()
{
    TreeBufs<Hdr, Counting> t;
    for (const TreeStep &s : kTreeSteps) {
        Reserved r = t.ensure(s.walkers, s.pops, s.depth, kTreeStride, kTreeGroups, kTreeHeavy);
        if (r.err) {
            CHECK(r.what[0] && r.bytes > 0);
            r = t.ensure(s.walkers, s.pops, s.depth, kTreeStride, kTreeGroups, kTreeHeavy);
            CHECK(!r.err);
        }
        check_tree(t, s);
    }
}

void tree_sequence_allocations()
{
    Counting::reset();
    {
        TreeBufs<Hdr, Counting> t;
        const TreeStep *s = kTreeSteps;
        CHECK(!t.ensure(s[0].walkers, s[0].pops, s[0].depth, kTreeStride, kTreeGroups, kTreeHeavy).err);
        CHECK(Counting::n_alloc == 4 && t.hdr_fresh && t.partial_fresh && t.par.capacity() == 224 * 12);
        // the same product walkers x pops, twice the candidates: the parameter rows grow (alone with the partial sums,
        // which follow the walkers too), headers and isochrones stay
        const Hdr *const hdr0 = t.hdr.get();
        CHECK(!t.ensure(s[1].walkers, s[1].pops, s[1].depth, kTreeStride, kTreeGroups, kTreeHeavy).err);
        CHECK(t.par.capacity() == 448 * 12 && t.hdr.get() == hdr0 && !t.hdr_fresh && t.partial_fresh && Counting::n_alloc == 6);
        check_tree(t, s[1]);
        CHECK(!t.ensure(s[2].walkers, s[2].pops, s[2].depth, kTreeStride, kTreeGroups, kTreeHeavy).err);
        CHECK(!t.ensure(s[3].walkers, s[3].pops, s[3].depth, kTreeStride, kTreeGroups, kTreeHeavy).err);
        CHECK(Counting::n_alloc == 6 && !t.hdr_fresh && !t.partial_fresh);        // nothing shrinks, nothing moves
        check_tree(t, s[3]);
        // a pack with another row length: the three candidate buffers start afresh, the partial sums stay
        CHECK(!t.ensure(2, 1, 2, kTreeStride + 2, kTreeGroups, kTreeHeavy).err);
        CHECK(Counting::n_alloc == 9 && t.hdr_fresh && !t.partial_fresh && t.iso_stride == kTreeStride + 2);
    }
    CHECK(Counting::live.empty());
}

// ---- the carve
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

void carve_checks()
{
    {   // the rule itself: in order, disjoint, aligned, and total = the sum of the rounded sizes
        Carve c;
        const size_t sizes[] = {1, 256, 257, 0, 1000, 8};
        size_t end = 0, sum = 0;
        for (size_t s : sizes) {
            const size_t o = c.take(s);
            CHECK(o % kArenaAlign == 0 && o >= end);
            end = o + s; sum += up256(s);
            CHECK(c.total >= end && c.total % kArenaAlign == 0);
        }
        CHECK(c.total == sum && kArenaAlign == 256);
    }
    // b9_sample_wd_mass through wd_grid_arena (its seven outputs are the scratch; no accumulators, no edges): the parts and the
    // total its body computed before any arena existed
    struct { size_t chunk; int n_pops; long long stride; size_t tab_row, n_wd, n; } wds[] = {{256, 2, 122 * 9, 40000, 37, 1000}, {3, 1, 62 * 5, 1234, 1, 13}};
    for (const auto &s : wds) {
        const size_t per = s.chunk * s.n_wd;
        const size_t o_hdr = up256(8 * B9_NPARAM * s.chunk), o_iso = o_hdr + up256(sizeof(Hdr) * s.chunk * s.n_pops);
        const size_t o_tab = o_iso + up256(8 * s.chunk * s.n_pops * (size_t)s.stride), o_out = o_tab + up256(8 * s.chunk * s.tab_row);
        const size_t o_pop = o_out + up256(8 * per * 7), o_rank = o_pop + up256(4 * per), bytes = o_rank + up256(4 * s.n);
        const WdGridArena a = wd_grid_arena(s.chunk, s.n_pops, s.stride, s.tab_row, s.n_wd, s.n, 7, 0, s.n_wd, 0, sizeof(Hdr));
        CHECK(a.o_par == 0 && a.o_hdr == o_hdr && a.o_iso == o_iso && a.o_tab == o_tab && a.o_scratch == o_out && a.o_pop == o_pop && a.o_rank == o_rank && a.bytes == bytes);
        CHECK(a.o_acc == a.o_pop && a.o_edges == a.bytes);                                              // the two empty parts
        const size_t offs[] = {a.o_par, a.o_hdr, a.o_iso, a.o_tab, a.o_scratch, a.o_pop, a.o_rank, a.bytes};
        for (int k = 0; k < 7; ++k) CHECK(offs[k] % 256 == 0 && offs[k] < offs[k + 1]);
    }
    // b9_wd_moments (16 words a star, no populations, no edges) and b9_wd_bins (6 and 1 selected quantities at 7 and 64 bins: n_lines
    // lines of n_bins + 3 words, n_bins + 1 edges a line) through the same function: in order, disjoint, aligned, an empty part
    // starts where the next one does, and the total is the sum of the rounded sizes -- for the moments [par][hdr][iso][tab][scratch]
    // [acc][rank], for the bins the same with [edges] behind, as the two calls' own arenas gave before this one
    struct { size_t chunk; int n_pops; long long stride; size_t tab_row, n_lines, n, n_col, n_edges; } wdg[] = {
        {256, 2, 122 * 9, 2 * 1000 * 23, 37, 1000, 16, 0}, {3, 1, 62 * 5, 1234, 1, 13, 16, 0},
        {64, 2, 122 * 9, 2 * 200 * 23, 37 * 6, 1000, 10, 8}, {5, 1, 122 * 17, 65 * 39, 3, 13, 67, 65},
    };
    for (const auto &s : wdg) {
        const WdGridArena a = wd_grid_arena(s.chunk, s.n_pops, s.stride, s.tab_row, s.n_lines, s.n, s.n_col, s.n_col, 0, s.n_edges, sizeof(Hdr));
        const size_t offs[] = {a.o_par, a.o_hdr, a.o_iso, a.o_tab, a.o_scratch, a.o_acc, a.o_pop, a.o_rank, a.o_edges, a.bytes};
        const size_t sizes[] = {8 * B9_NPARAM * s.chunk, sizeof(Hdr) * s.chunk * s.n_pops, 8 * s.chunk * s.n_pops * (size_t)s.stride, 8 * s.chunk * s.tab_row,
                                8 * s.chunk * s.n_lines * s.n_col, 8 * s.n_lines * s.n_col, 0, 4 * s.n, 8 * s.n_lines * s.n_edges};
        CHECK(a.o_par == 0);
        for (int k = 0; k < 9; ++k) {
            CHECK(offs[k] % 8 == 0 && offs[k] % kArenaAlign == 0);
            CHECK(offs[k] + sizes[k] <= offs[k + 1] && offs[k + 1] == offs[k] + up256(sizes[k]));      // disjoint, in order, no slack beyond the rounding
            if (sizes[k] == 0) CHECK(offs[k] == offs[k + 1]);                                           // an empty part
        }
        CHECK(a.o_pop == a.o_rank);
        const size_t moments = up256(sizes[0]) + up256(sizes[1]) + up256(sizes[2]) + up256(sizes[3]) + up256(sizes[4]) + up256(sizes[5]) + up256(sizes[7]);
        CHECK(a.bytes == moments + up256(sizes[8]) && a.o_edges == moments);
        if (s.n_edges == 0) CHECK(a.bytes == moments);
    }
    // the reductions over a saved chain: the four calls' shapes (moments; hist with row sums; resid with its three extra parts;
    // pointwise with flags and two tails), a call without WD-stage stars, and one without a tail or row sums.  Every part lies
    // on an 8-byte (in fact 256-byte) boundary, holds its bytes without reaching the next one, and `bytes` is the end of the
    // last part; a part of 0 bytes is empty -- it starts where the next one does.
    struct { size_t chunk; int n_pops; long long stride; size_t tab_row, wd_row, n, n_col, n_acc, n_rowcol, extra[kChainExtras]; } chain[] = {
        {32, 2, 122 * 9, 40000, 2 * 32 * 17, 1000, 8, 8, 0, {0, 0, 0}},
        {32, 1, 62 * 5, 1234, 32 * 9, 13, 34, 34, 34, {0, 0, 0}},
        {7, 2, 122 * 17, 5000, 2 * 32 * 33, 130, 34, 34, 81, {8 * 130 * 16, 8 * 192 * 16, 8 * 130 * 16}},
        {32, 1, 122 * 9, 40000, 32 * 17, 1000, 1, 8, 1, {4 * 32, 8 * 1000 * 5, 8 * 1000 * 5}},
        {32, 1, 122 * 9, 40000, 0, 1000, 1, 8, 1, {4 * 32, 8 * 1000 * 5, 8 * 1000 * 5}},       // wd_row = 0
        {32, 1, 122 * 9, 40000, 32 * 17, 1000, 1, 8, 0, {4 * 32, 0, 0}},                      // tail_len = 0, no row sums
    };
    for (const auto &s : chain) {
        const ChainArena a = chain_arena(s.chunk, s.n_pops, s.stride, s.tab_row, s.wd_row, s.n, s.n_col, s.n_acc, s.n_rowcol, sizeof(Hdr), s.extra);
        const size_t offs[] = {a.o_par, a.o_hdr, a.o_iso, a.o_tab, a.o_wd, a.o_scratch, a.o_acc, a.o_rows, a.o_extra[0], a.o_extra[1], a.o_extra[2], a.bytes};
        const size_t sizes[] = {8 * B9_NPARAM * s.chunk, sizeof(Hdr) * s.chunk * s.n_pops, 8 * s.chunk * s.n_pops * (size_t)s.stride, 8 * s.chunk * s.tab_row,
                                8 * s.chunk * s.wd_row, 8 * s.chunk * s.n * s.n_col, 8 * s.n * s.n_acc, 8 * s.chunk * s.n_rowcol,
                                s.extra[0], s.extra[1], s.extra[2]};
        CHECK(a.o_par == 0);
        for (int k = 0; k < 11; ++k) {
            CHECK(offs[k] % 8 == 0 && offs[k] % kArenaAlign == 0);
            CHECK(offs[k] + sizes[k] <= offs[k + 1] && offs[k + 1] == offs[k] + up256(sizes[k]));      // disjoint, in order, no slack beyond the rounding
            if (sizes[k] == 0) CHECK(offs[k] == offs[k + 1]);                                           // an empty part
        }
        CHECK(a.bytes == a.o_extra[2] + up256(s.extra[2]));
    }
    CHECK(mom_chunk_rows(33, 130, 8, 32, (size_t)64 << 20) == 32 && mom_chunk_rows(5, 130, 8, 32, (size_t)64 << 20) == 5);
    CHECK(mom_chunk_rows(33, 1 << 20, 8, 32, (size_t)64 << 20) == 1 && mom_chunk_rows(33, 0, 8, 32, (size_t)64 << 20) == 32);
    // b9_predict_mags: its body laid the six parts back to back (8c, 8c, 8c nf, 4c, 4c, 4c bytes).  Whole chunks of 2^20
    // systems -- every chunk but a catalogue's last -- and any chunk that is a multiple of 64 systems have every part on a
    // 256-byte boundary already: same offsets, same total.  Any other count gains less than 256 bytes of padding per part.
    struct { size_t chunk; int nf; bool same; } pred[] = {{(size_t)1 << 20, 8, true}, {4096, 5, true}, {1000, 3, false}};
    for (const auto &s : pred) {
        const size_t o_q = 8 * s.chunk, o_mags = 2 * o_q, o_wd = o_mags + 8 * s.chunk * s.nf, o_pop = o_wd + 4 * s.chunk, o_stage = o_pop + 4 * s.chunk;
        const size_t bytes = o_stage + 4 * s.chunk;
        const PredArena a = pred_arena(s.chunk, s.nf);
        const size_t offs[] = {a.o_m1, a.o_q, a.o_mags, a.o_wd, a.o_pop, a.o_stage, a.bytes};
        const size_t sizes[] = {8 * s.chunk, 8 * s.chunk, 8 * s.chunk * s.nf, 4 * s.chunk, 4 * s.chunk, 4 * s.chunk};
        for (int k = 0; k < 6; ++k) CHECK(offs[k] % 256 == 0 && offs[k] + sizes[k] <= offs[k + 1]);
        if (s.same) CHECK(a.o_m1 == 0 && a.o_q == o_q && a.o_mags == o_mags && a.o_wd == o_wd && a.o_pop == o_pop && a.o_stage == o_stage && a.bytes == bytes);
        else CHECK(a.bytes >= bytes && a.bytes < bytes + 6 * 256);
    }
}

void sizing_checks()
{
    CHECK(pack_mass_cap(119) == 120 && pack_mass_cap(120) == 120 && pack_mass_cap(121) == 122);       // (max_eep + 1) & ~1
    CHECK(pack_iso_stride(120, 8) == 120 * 9);
    const WorkNeed w = work_need(8, 2, 120, 8);
    CHECK(w.hdr == 64 && w.iso == (size_t)1080 * 64 && w.params == (size_t)12 * 8 * 4 && w.logpost == 8);
    // candidate c of parity p of a fused block: the expressions its callers wrote out (set c0 = 2 p + c of [2][2] sets, W walkers
    // each: W parameter rows, rows = W n_pops headers / isochrones / node tables)
    for (int W : {1, 3})
        for (int n_pops : {1, 2})
            for (int p = 0; p < 2; ++p)
                for (int c = 0; c < 2; ++c) {
                    const size_t rows = (size_t)W * n_pops, c0 = (size_t)p * 2 + c;
                    const CandAt at = cand_at(p, c, W, n_pops);
                    CHECK(at.row == c0 * W && at.wp == c0 * rows);
                    CHECK(at.row * B9_NPARAM == c0 * W * B9_NPARAM);                                  // parameter doubles
                    const size_t stride = (size_t)pack_iso_stride(120, 8), tab = 977, wd_stride = rows * 33;
                    CHECK(at.wp * stride == c0 * rows * stride && at.wp * tab == c0 * rows * tab);     // isochrone and node-table doubles
                    CHECK(at.wp * 33 == c0 * wd_stride);                                               // WD tables: wd_stride a candidate
                    if (c == 0) CHECK(at.row == (size_t)p * 2 * W && at.wp == (size_t)p * 2 * rows);   // k_marg_step's c0 = set * 2
                }
    CHECK(cand_at(1, 0, 3, 2).row == 6 && cand_at(1, 0, 3, 2).wp == 12 && cand_at(0, 0, 3, 2).wp == 0 && cand_at(1, 1, 1, 1).row == 3);
    CHECK(tree_part_stride(3, 4) == 16 && tree_part_stride(3, 5) == 18);
    const TreeNeed t = tree_need(2, 2, 3, 100, 3, 4);
    CHECK(t.n_cand == 224 && t.hdr == 448 && t.iso == 44800 && t.par == 224 * 12 && t.partial == (size_t)2 * 2 * 7 * 16);
}

int main()
{
    sizing_checks();
    carve_checks();
    const int n_buf = at_every_failure_point(buf_scenario);
    const int n_up = at_every_failure_point(upload_scenario);
    upload_copy_failure();
    const int n_work = at_every_failure_point(work_scenario);
    work_sequence_allocations();
    const int n_tree = at_every_failure_point(tree_scenario);
    tree_sequence_allocations();
    CHECK(Counting::live.empty());
    std::printf("devbuf_host: ok (failure points walked: buf %d, uploads %d, work group %d, tree group %d)\n", n_buf, n_up, n_work, n_tree);
    return 0;
}
