// CPU-only check of every workspace carve function (csrc/p2w_ws.h), meant for a sanitizer build of the HOST code:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I include -Xarch_host -fsanitize=address,undefined \
//         tools/ws_layout_check.cpp -o ws_layout_check && ./ws_layout_check
//
// For a grid of sizes it runs each carve function on a malloc'ed buffer of exactly bytes() and checks that every region it
// hands out lies inside the buffer, is aligned for its element type (workspaces are 16-byte aligned, as malloc's are) and
// overlaps no other; then it writes every byte of every region, which AddressSanitizer watches.  No kernel is launched and
// no device is opened.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Region { char* p; size_t n, type_align; };
static std::vector<Region> g_regions;
#define P2W_WS_TRACE(p, n, type_align) do { if (p) g_regions.push_back({static_cast<char*>(p), (n), (type_align)}); } while (0)

#include "../pointstowood_amd/csrc/p2w_geom.hip"
#include "../pointstowood_amd/csrc/p2w_feat.hip"
#include "../pointstowood_amd/csrc/p2w_feat_h1.hip"
#include "../pointstowood_amd/csrc/p2w_cluster.hip"
#include "../pointstowood_amd/csrc/p2w_pathlen.hip"
#include "../pointstowood_amd/csrc/p2w_eval.hip"
#include "../pointstowood_amd/csrc/p2w_grad.hip"
#include "../pointstowood_amd/csrc/p2w_loss.hip"
#include "../pointstowood_amd/csrc/p2w_edge.hip"
#include "../pointstowood_amd/csrc/p2w_bnmax.hip"
#include "../pointstowood_amd/csrc/p2w_bnchain.hip"
#include "../pointstowood_amd/csrc/p2w_fp.hip"
#include "../pointstowood_amd/csrc/p2w_head.hip"
#include "../pointstowood_amd/csrc/p2w_feed.hip"
#include "../pointstowood_amd/csrc/p2w_sample.hip"
#include "../pointstowood_amd/csrc/p2w_optim.hip"

static int g_fail = 0, g_runs = 0;

template <class Carve> static void check(const char* name, long long x, long long y, long long z, Carve carve) {
    P2wArena measure;
    carve(measure);
    const size_t bytes = measure.bytes();
    char* buf = static_cast<char*>(malloc(bytes));
    g_regions.clear();
    P2wArena arena(buf);
    carve(arena);
    auto bad = [&](const char* what, const Region& r) {
        ++g_fail;
        printf("FAIL %s(%lld, %lld, %lld): %s: region at %td, %zu bytes, element alignment %zu, workspace %zu bytes\n", name, x, y, z, what,
               r.p - buf, r.n, r.type_align, bytes);
    };
    if (arena.bytes() != bytes) bad("sizes differ between the two runs", Region{buf, arena.bytes(), 1});
    std::vector<Region> rs;
    for (const Region& r : g_regions) if (r.n) rs.push_back(r);                     // (an empty region touches nothing)
    std::sort(rs.begin(), rs.end(), [](const Region& a, const Region& b) { return a.p < b.p; });
    for (size_t i = 0; i < rs.size(); ++i) {
        const Region& r = rs[i];
        if (r.p < buf || r.p + r.n > buf + bytes) bad("outside the buffer", r);
        if (r.type_align > 16 || reinterpret_cast<uintptr_t>(r.p) % r.type_align) bad("misaligned for its type", r);
        if (i + 1 < rs.size() && r.p + r.n > rs[i + 1].p) bad("overlaps the next region", r);
    }
    for (const Region& r : g_regions) memset(r.p, 0x5a, r.n);
    free(buf);
    ++g_runs;
}

int main() {
    const long long sizes[] = {0, 1, 3, 4, 5, 255, 256, 257, 1025, 4097, 100003, 2000000};
    for (long long n : sizes) {
        const int i = (int)n;
        check("rs_carve", n, 0, 0, [&](P2wArena& a) { rs_carve(a, n); });
        check("xs_carve", n, 0, 0, [&](P2wArena& a) { xs_carve(a, n); });
        if (n > 0) check("vs_carve", n, 0, 0, [&](P2wArena& a) { vs_carve(a, i); });
        if (n > 0) check("mo_carve", n, 0, 0, [&](P2wArena& a) { mo_carve(a, i); });
        check("vr_carve", n, 0, 0, [&](P2wArena& a) { vr_carve(a, i); });
        check("ec_carve", n, 0, 0, [&](P2wArena& a) { ec_carve(a, n); });
        check("grow_carve", n, 0, 0, [&](P2wArena& a) { grow_carve(a, n); });
        check("lf_carve", n, 0, 0, [&](P2wArena& a) { lf_carve(a, n); });
        check("sm_carve", n, 0, 0, [&](P2wArena& a) { sm_carve(a, n); });
        check("op_carve", n, 0, 0, [&](P2wArena& a) { op_carve(a, n); });
        for (int flags : {0, (int)P2W_SA_PACK8}) check("sa_conv_carve", n, flags, 0, [&](P2wArena& a) { sa_conv_carve(a, (long)n, flags); });
        for (long long t : {0ll, 1ll, 257ll, 4097ll, 1ll << 22}) {
            check("tk_carve", n, t, 0, [&](P2wArena& a) { tk_carve(a, i, t); });
            check("sssp_carve", n, t, 0, [&](P2wArena& a) { sssp_carve(a, n, t); });
        }
        for (int N : {1, 64, 65, 256}) check("rowdot_carve", n, N, 0, [&](P2wArena& a) { rowdot_carve(a, i, N); });
        for (int B : {0, 1, 3, 257}) check("fd_carve", n, B, 0, [&](P2wArena& a) { fd_carve(a, n, B); });
        for (long long S : {0ll, 1ll, 300ll, 4095ll, 4096ll}) check("cp_carve", n, S, 0, [&](P2wArena& a) { cp_carve(a, n, S); });
        for (int s : {1, 3, 7})
            for (int c : {2, 3, 8}) check("ev_carve", n, s, c, [&](P2wArena& a) { ev_carve(a, n, s, c); });
        for (int rows : {0, 1, 2, 257}) {
            check("ib_carve", n, rows, 0, [&](P2wArena& a) { ib_carve(a, n, rows); });
            if (n <= 100003) check("fp_carve", n, rows, 0, [&](P2wArena& a) { fp_carve(a, i, 3, rows); });
            for (int C : {1, 32, 33, 67}) {
                check("eb_carve", n, rows, C, [&](P2wArena& a) { eb_carve(a, i, rows, C); });
                if (n > 0) check("bm_carve", n, C, 0, [&](P2wArena& a) { bm_carve(a, i, C); });
                if (n > 1 && rows == 1)
                    for (int L = 1; L <= P2W_BN_CHAIN_MAX; ++L) check("bc_carve", n, C, L, [&](P2wArena& a) { bc_carve(a, i, C, L); });
                if (n > 1 && rows == 1) check("hd_carve", n, C, 0, [&](P2wArena& a) { hd_carve(a, i, C); });
            }
        }
    }
    printf("%d layouts checked, %d failures\n", g_runs, g_fail);
    return g_fail ? 1 : 0;
}
