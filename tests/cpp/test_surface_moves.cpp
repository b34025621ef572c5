// test_surface_moves.cpp -- the moves of the resident surfaces (csrc/surface_rules.h: surface_plan_moves; surface_device.h) on their own: the rule
// headers and the standard library, nothing of the engine, no GPU.  It keeps a store and a bounce buffer in host memory and runs a script of
// defines, keyframes and move calls; for every call it prints the verdict, each move's phase and path, the phases and the job and band tables, and
// EXECUTES the phases' launches item by item as the kernels walk them (surface_device.h: surface_band_item, surface_move_item; launch B through the
// patch kernel's walk) -- THREE times: items in table order, in reverse, and in a seeded shuffle.  A launch is correct whatever order its workgroups
// run in exactly if the three stores agree, no destination byte is written twice in a launch, and launch A reads no store byte that it writes; the
// walk checks all of that, the alignment of every wide store, and that no access leaves its row.  tests/test_surface_moves.py drives it and compares
// the store with the numpy oracle.  TEST INFRASTRUCTURE.
//
//   test_surface_moves SCRIPT      one command per line:
//       store MAX_SURFACES MAX_BYTES_EACH
//       define S FMT W H
//       keyframe S FILE            the surface's tight bytes; makes the slot valid
//       bounce BYTES               the bounce buffer (zly_surface_moves_enable)
//       moves N                    then N lines "S SX SY DX DY W H"
//       moves_null N               a call with a null array
//       dump S FILE                the slot's whole stride
#include "surface_rules.h"

#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <sstream>
#include <vector>

using namespace zly;

static const uint8_t POISON = 0xEE;       // what the host store holds before anything is written
static const uint8_t BOUNCE_POISON = 0x77;

struct World {
    SurfaceStore st;
    std::vector<SurfaceSlot> slots;
    std::vector<uint8_t> store;
    size_t bounce_bytes = 0;
    bool enabled = false;
};

struct Item { uint32_t band; uint64_t i; };

static uint32_t g_seed = 2463534242u;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5; return g_seed; }

// order 0: as the table has them; 1: reversed; 2: shuffled
static void reorder(std::vector<Item>* items, int order)
{
    if (order == 1) std::reverse(items->begin(), items->end());
    if (order == 2) for (size_t k = items->size(); k > 1; --k) std::swap((*items)[k - 1], (*items)[rnd() % k]);
}

// k bytes from src[s..] to dst[d..] as a lane writes them: one 16-byte store, or the clipped granule's naturally aligned stores; the violations
static int copy_granule(const std::vector<uint8_t>& src, uint64_t s, std::vector<uint8_t>* dst, uint64_t d, uint32_t k, std::vector<uint8_t>* wrote, std::vector<uint8_t>* read)
{
    int bad = 0;
    if (k < 1 || k > 16 || s + k > src.size() || d + k > dst->size()) return 1;
    uint8_t tmp[16];
    memcpy(tmp, src.data() + s, k);                          // a lane loads its granule whole before it stores
    if (read) for (uint32_t t = 0; t < k; ++t) (*read)[s + t] = 1;
    uint32_t at = 0;
    while (k) {
        const uint32_t wd = (k == 16 && at == 0) ? 16 : surface_edge_width((uint32_t)d, k);
        if (d % wd || wd > k) ++bad;
        for (uint32_t t = 0; t < wd; ++t) { (*dst)[d + t] = tmp[at + t]; if ((*wrote)[d + t]++) ++bad; }      // no byte is written twice in a launch
        d += wd; at += wd; k -= wd;
    }
    return bad;
}

// launch A: surface_move_kernel's walk over bands [first, first + count)
static int launch_a(const SurfaceMoveBand* bands, size_t count, int order, std::vector<uint8_t>* store, std::vector<uint8_t>* bounce, std::vector<uint8_t>* bounce_set)
{
    int bad = 0;
    std::vector<Item> items;
    for (size_t b = 0; b < count; ++b) {
        const uint64_t n = (uint64_t)bands[b].rows * surface_row_granules(bands[b].row_bytes);
        for (uint64_t i = 0; i < n; ++i) items.push_back({(uint32_t)b, i});
    }
    reorder(&items, order);
    std::vector<uint8_t> wrote_store(store->size(), 0), wrote_bounce(bounce->size(), 0), read(store->size(), 0);
    for (const Item& it : items) {
        const SurfaceMoveBand& j = bands[it.band];
        uint32_t r, g, k;
        surface_band_item(j.rows, surface_row_granules(j.row_bytes), it.i, &r, &g);
        uint64_t s, d;
        if (r >= j.rows) { ++bad; continue; }
        if (!surface_move_item(j, r, g, &s, &d, &k)) continue;
        const uint64_t srow = j.src_off + (uint64_t)r * j.src_pitch, drow = surface_move_dst(j) + (uint64_t)r * j.dst_pitch;
        if (s < srow || s + k > srow + j.row_bytes || d < drow || d + k > drow + j.row_bytes || s - srow != d - drow) { ++bad; continue; }    // inside its row, on both sides
        const bool tb = surface_move_to_bounce(j);
        bad += copy_granule(*store, s, tb ? bounce : store, d, k, tb ? &wrote_bounce : &wrote_store, &read);
    }
    for (size_t i = 0; i < store->size(); ++i) bad += read[i] && wrote_store[i];     // the launch reads no byte that it writes
    for (size_t i = 0; i < bounce->size(); ++i) if (wrote_bounce[i]) (*bounce_set)[i] = 1;
    return bad;
}

// launch B: surface_patch_kernel's walk, the bounce buffer as its staging
static int launch_b(const SurfaceJob* bands, size_t count, int order, const std::vector<uint8_t>& bounce, const std::vector<uint8_t>& bounce_set, std::vector<uint8_t>* store)
{
    int bad = 0;
    std::vector<Item> items;
    for (size_t b = 0; b < count; ++b) {
        const uint64_t n = (uint64_t)bands[b].rows * surface_row_granules(bands[b].row_bytes);
        for (uint64_t i = 0; i < n; ++i) items.push_back({(uint32_t)b, i});
    }
    reorder(&items, order);
    std::vector<uint8_t> wrote(store->size(), 0);
    for (const Item& it : items) {
        const SurfaceJob& j = bands[it.band];
        const uint32_t n = j.row_bytes, G = surface_row_granules(n);
        const uint32_t r = j.rows == 1 ? 0 : (uint32_t)it.i / G, g = j.rows == 1 ? (uint32_t)it.i : (uint32_t)it.i - r * G;
        const uint64_t drow = j.dst_off + (uint64_t)r * j.pitch;
        uint32_t lo, hi;
        if (!surface_granule(drow, n, g, &lo, &hi)) continue;
        if (hi > n || lo >= hi) { ++bad; continue; }
        const uint64_t s = j.src_off + (uint64_t)r * n + lo;
        for (uint32_t t = 0; t < hi - lo && s + t < bounce_set.size(); ++t) bad += !bounce_set[s + t];       // only what this phase gathered
        bad += copy_granule(bounce, s, store, drow + lo, hi - lo, &wrote, nullptr);
    }
    return bad;
}

static int execute(const SurfaceMovePlan& pl, int order, size_t bounce_bytes, std::vector<uint8_t>* store)
{
    int bad = 0;
    for (const SurfaceMovePhase& ph : pl.phases) {
        std::vector<uint8_t> bounce(bounce_bytes, BOUNCE_POISON), bounce_set(bounce_bytes, 0);
        bad += launch_a(pl.a_bands.data() + ph.a_first, ph.a_count, order, store, &bounce, &bounce_set);
        bad += launch_b(pl.b_bands.data() + ph.b_first, ph.b_count, order, bounce, bounce_set, store);
        bad += ph.bounce_bytes > bounce_bytes;
    }
    return bad;
}

// the tables' own shape: bands tile their jobs in job order, bounce jobs start 16-byte aligned and stay inside the phase's share, phases are consecutive
static int check_tables(const SurfaceMovePlan& pl, int n_moves)
{
    int bad = 0;
    size_t k = 0;
    for (const SurfaceMoveBand& j : pl.a_jobs) {
        uint32_t r = 0;
        while (r < j.rows) {
            if (k >= pl.a_bands.size()) return bad + 1;
            const SurfaceMoveBand& b = pl.a_bands[k++];
            if (b.row_bytes != j.row_bytes || b.src_pitch != j.src_pitch || b.dst_pitch != j.dst_pitch || b.rows < 1 || b.src_off != j.src_off + (uint64_t)r * j.src_pitch ||
                b.dst_off != j.dst_off + (uint64_t)r * j.dst_pitch) ++bad;
            if (b.rows > 1 && (uint64_t)b.rows * b.row_bytes > ZLY_SURFACE_BAND_BYTES) ++bad;
            if (r + b.rows < j.rows && (uint64_t)(b.rows + 1) * b.row_bytes <= ZLY_SURFACE_BAND_BYTES) ++bad;
            r += b.rows;
        }
        if (surface_move_to_bounce(j) && (surface_move_dst(j) % 16 || j.dst_pitch != j.row_bytes)) ++bad;
    }
    bad += k != pl.a_bands.size();
    k = 0;
    for (const SurfaceJob& j : pl.b_jobs) {
        uint32_t r = 0;
        while (r < j.rows) {
            if (k >= pl.b_bands.size()) return bad + 1;
            const SurfaceJob& b = pl.b_bands[k++];
            if (b.row_bytes != j.row_bytes || b.pitch != j.pitch || b.src_off != j.src_off + (uint64_t)r * j.row_bytes || b.dst_off != j.dst_off + (uint64_t)r * j.pitch) ++bad;
            if (b.rows > 1 && (uint64_t)b.rows * b.row_bytes > ZLY_SURFACE_BAND_BYTES) ++bad;
            r += b.rows;
        }
        bad += j.src_off % 16 != 0;
    }
    bad += k != pl.b_bands.size();
    int32_t next = 0; size_t na = 0, nb = 0;
    for (const SurfaceMovePhase& ph : pl.phases) {
        bad += ph.first != next || ph.a_first != na || ph.b_first != nb;
        next += ph.count; na += ph.a_count; nb += ph.b_count;
    }
    bad += next != n_moves || na != pl.a_bands.size() || nb != pl.b_bands.size();
    bad += pl.table_bytes != 32 * (pl.a_bands.size() + pl.b_bands.size());
    return bad;
}

static void run_moves(World& W, int n, const SurfaceMoveReq* moves)
{
    SurfaceMovePlan pl;
    std::string err;
    const int rc = surface_plan_moves(W.st, W.slots.data(), n, moves, W.bounce_bytes, &pl, &err);
    if (rc != ZLY_OK) { printf("moves %d\nerror %s\n", rc, err.c_str()); return; }
    printf("moves 0 %zu %zu %zu %zu %zu %zu\n", pl.phases.size(), pl.a_jobs.size(), pl.a_bands.size(), pl.b_jobs.size(), pl.b_bands.size(), pl.table_bytes);
    for (int i = 0; i < n; ++i) printf("move %d %d %d\n", i, pl.phase_of[(size_t)i], (int)pl.via[(size_t)i]);
    for (const SurfaceMovePhase& ph : pl.phases)
        printf("phase %d %d %zu %zu %zu %zu %zu\n", ph.first, ph.count, ph.a_first, ph.a_count, ph.b_first, ph.b_count, ph.bounce_bytes);
    for (int t = 0; t < 2; ++t)
        for (const SurfaceMoveBand& j : t ? pl.a_bands : pl.a_jobs)
            printf("%s %llu %llu %d %u %u %u %u\n", t ? "aband" : "ajob", (unsigned long long)j.src_off, (unsigned long long)surface_move_dst(j), (int)surface_move_to_bounce(j), j.row_bytes,
                   j.rows, j.src_pitch, j.dst_pitch);
    for (int t = 0; t < 2; ++t)
        for (const SurfaceJob& j : t ? pl.b_bands : pl.b_jobs)
            printf("%s %llu %llu %u %u %u\n", t ? "bband" : "bjob", (unsigned long long)j.src_off, (unsigned long long)j.dst_off, j.row_bytes, j.rows, j.pitch);
    std::vector<uint8_t> out[3];
    int bad = check_tables(pl, n);
    for (int order = 0; order < 3; ++order) {
        out[order] = W.store;
        bad += execute(pl, order, W.bounce_bytes, &out[order]);
    }
    const bool same = out[0] == out[1] && out[0] == out[2];
    W.store = out[2];
    printf("exec %s %d\n", same ? "same" : "DIFFER", bad);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: test_surface_moves SCRIPT\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    World W;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd) || cmd[0] == '#') continue;
        std::string err;
        if (cmd == "store") {
            long long s = 0; unsigned long long b = 0;
            in >> s >> b;
            SurfaceStore st;
            const int rc = W.enabled ? ZLY_ERR_INVALID_ARGUMENT : surfaces_plan_store((int32_t)s, (size_t)b, &st, &err);
            if (rc == ZLY_OK && st.total <= (1u << 28)) { W.st = st; W.slots.assign((size_t)s, SurfaceSlot()); W.store.assign(st.total, POISON); W.enabled = true; }
            printf("store %d %zu %zu\n", rc, rc ? (size_t)0 : st.stride, rc ? (size_t)0 : st.total);
        } else if (cmd == "define") {
            int s = 0, fmt = 0, w = 0, h = 0;
            in >> s >> fmt >> w >> h;
            SurfaceSlot sl;
            const int rc = surface_define(W.st, s, fmt, w, h, &sl, &err);
            if (rc == ZLY_OK) W.slots[(size_t)s] = sl;
            printf("define %d\n", rc);
        } else if (cmd == "keyframe") {
            int s = 0; std::string file;
            in >> s >> file;
            std::ifstream pf(file, std::ios::binary);
            std::vector<uint8_t> px((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
            int rc = surface_check_slot(W.st, s, &err);
            if (rc == ZLY_OK && (!W.slots[(size_t)s].defined || px.size() != frame_bytes(W.slots[(size_t)s].fmt, W.slots[(size_t)s].w, W.slots[(size_t)s].h))) rc = ZLY_ERR_INVALID_ARGUMENT;
            if (rc == ZLY_OK) { memcpy(W.store.data() + (size_t)s * W.st.stride, px.data(), px.size()); W.slots[(size_t)s].valid = true; }
            printf("keyframe %d\n", rc);
        } else if (cmd == "bounce") {
            unsigned long long b = 0;
            in >> b;
            W.bounce_bytes = (size_t)b;
            printf("bounce 0\n");
        } else if (cmd == "moves" || cmd == "moves_null") {
            int n = 0;
            in >> n;
            std::vector<SurfaceMoveReq> ms;
            for (int i = 0; cmd == "moves" && i < n && std::getline(f, line); ++i) {
                std::istringstream q(line);
                SurfaceMoveReq m{};
                q >> m.surface >> m.sx >> m.sy >> m.dx >> m.dy >> m.w >> m.h;
                ms.push_back(m);
            }
            if (cmd == "moves" && ms.empty()) ms.push_back(SurfaceMoveReq{});
            run_moves(W, n, cmd == "moves" ? ms.data() : nullptr);
        } else if (cmd == "dump") {
            int s = 0; std::string file;
            in >> s >> file;
            std::ofstream of(file, std::ios::binary);
            of.write((const char*)W.store.data() + (size_t)s * W.st.stride, (std::streamsize)W.st.stride);
            printf("dump %d\n", s);
        } else {
            printf("unknown %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
