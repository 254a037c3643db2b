// Stand-alone check of the host layer the convolution files share (radar_depth_amd/csrc/conv_host.h): the plan cache, its key, the
// plan-all switch and the descriptor checks build without the HIP runtime, so they can run under the host sanitizers.  Eight threads
// hammer one cache with find / insert / epoch bumps and the tuner's pin / commit on twenty synthetic descriptors; every entry a find
// returns must be one that was inserted whole, a plan handed out must never be replaced, and a stale tile_begin must not make a
// second key.  Build and run once per sanitizer, as a plain executable:
//   c++ -std=c++17 -O1 -g -fsanitize=thread -pthread -o /tmp/conv_host_check tools/conv_host_check.cpp radar_depth_amd/csrc/conv_host.cpp && /tmp/conv_host_check
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -o /tmp/conv_host_check tools/conv_host_check.cpp radar_depth_amd/csrc/conv_host.cpp && /tmp/conv_host_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>

#include "../radar_depth_amd/csrc/conv_host.h"

namespace rd {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace rd
using namespace rd;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static RdConvDesc make_desc(int id) {       // a 3x3 convolution whose size encodes id
    RdConvDesc d;
    memset(&d, 0, sizeof(d));
    d.N = 2; d.Hi = d.Ho = 8 + id; d.Wi = d.Wo = 12 + id; d.Cin = d.ldi = 32; d.Cout = d.ldo = 64;
    d.in_stride = d.out_stride = 1; d.n_phases = 1;
    RdPhase& p = d.phase[0];
    p.n_taps = 9; p.lh = d.Ho; p.lw = d.Wo; p.dh_min = p.dw_min = -1; p.dh_max = p.dw_max = 1;
    for (int t = 0; t < 9; ++t) { p.dh[t] = (int8_t)(t / 3 - 1); p.dw[t] = (int8_t)(t % 3 - 1); p.widx[t] = (int16_t)t; }
    return d;
}

// an entry is whole when every word of it tells the same (id, version)
struct Entry { int id, version, tuner_owned; int fill[64]; };
static Entry make_entry(int id, int version, int owned) {
    Entry e;
    e.id = id; e.version = version; e.tuner_owned = owned;
    for (int i = 0; i < 64; ++i) e.fill[i] = id * 1000 + version;
    return e;
}
static bool whole(const Entry& e, int id) {
    if (e.id != id) return false;
    for (int i = 0; i < 64; ++i)
        if (e.fill[i] != id * 1000 + e.version) return false;
    return true;
}

static int no_domain(const RdConvDesc&) { return RD_OK; }

int main() {
    constexpr int N_DESC = 20, N_THREADS = 8, ITERS = 4000;
    // ---- single-threaded: checks, key, helpers
    RdConvDesc d0 = make_desc(0);
    REQUIRE(desc_taps_ok(d0) && desc_taps_ok(d0, 9) && !desc_taps_ok(d0, 8));
    REQUIRE(check_desc(&d0, "t", no_domain) == RD_OK && check_desc(nullptr, "t", no_domain) == RD_EINVAL && !strcmp(g_err, "t: null descriptor"));
    { RdConvDesc b = d0; b.phase[0].dw[2] = 3; REQUIRE(!desc_taps_ok(b) && check_desc(&b, "t", no_domain) == RD_EINVAL && !strcmp(g_err, "t: tap 2 of phase 0 outside its declared range")); }
    { RdConvDesc b = d0; b.n_phases = 5; REQUIRE(!desc_taps_ok(b) && check_desc(&b, "t", no_domain) == RD_EINVAL && !strcmp(g_err, "t: n_phases=5")); }
    { RdConvDesc b = d0; b.phase[0].lh = 0; REQUIRE(!desc_taps_ok(b) && check_desc(&b, "t", no_domain) == RD_EINVAL && !strcmp(g_err, "t: empty phase 0")); }
    { RdConvDesc b = d0; for (int i = 0; i < RD_MAX_PHASES; ++i) b.phase[i].tile_begin = 7 + i; REQUIRE(plan_key(b, {1}) == plan_key(d0, {1})); }
    REQUIRE(plan_key(d0, {1}) != plan_key(d0, {0}) && plan_key(d0) != plan_key(make_desc(1)) && plan_key(d0, {1, 2}).size() == sizeof(RdConvDesc) + 8);
    REQUIRE(weight_slabs(d0) == 9);
    { RdConvDesc b = d0; b.n_phases = 2; b.phase[1] = b.phase[0]; REQUIRE(fill_tile_begin(b, 4, 4) == 12 && b.phase[0].tile_begin == 0 && b.phase[1].tile_begin == 6); }
    { int tb[RD_MAX_PHASES + 1]; REQUIRE(fill_row_tile_begin(d0, 128, tb) == 2 && tb[0] == 0 && tb[1] == 2 && tb[RD_MAX_PHASES] == 2); }
    {
        alignas(16) float buf[8];
        REQUIRE(epilogue_vec4_ok(buf, 64, 64, 0, nullptr, 0, nullptr, 4) && !epilogue_vec4_ok(buf + 1, 64, 64, 0, nullptr, 0, nullptr, 4));
        REQUIRE(epilogue_vec4_ok(buf + 2, 64, 64, 4, buf, 8, buf, 2) && !epilogue_vec4_ok(buf + 2, 64, 64, 4, buf, 8, buf, 4) && !epilogue_vec4_ok(buf, 64, 62, 0, nullptr, 0, nullptr, 4));
    }
    static PlanAllSwitch sw([]() { return false; });
    unsigned ep = 99;
    REQUIRE(!sw.get(&ep) && ep == 0 && sw.set(1) == 0 && sw.get(&ep) && ep == 1 && sw.set(1) == 1 && sw.get(&ep) && ep == 1 && sw.set(0) == 1 && !sw.get(&ep) && ep == 2);

    // ---- eight threads on one cache
    static PlanCache<Entry> cache;
    static std::atomic<long> finds{0}, hits{0}, pins{0}, refused{0};
    RdConvDesc descs[N_DESC];
    for (int i = 0; i < N_DESC; ++i) descs[i] = make_desc(i);
    std::thread th[N_THREADS];
    for (int t = 0; t < N_THREADS; ++t)
        th[t] = std::thread([t, &descs]() {
            unsigned seed = 12345u + 977u * t;
            auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
            for (int it = 0; it < ITERS; ++it) {
                const int id = rnd() % N_DESC, op = rnd() % 16;
                RdConvDesc d = descs[id];
                d.phase[rnd() % RD_MAX_PHASES].tile_begin = (int)(rnd() % 100);      // (a caller's stale value)
                const std::string key = plan_key(d, {1});
                unsigned epoch;
                sw.get(&epoch);
                if (op == 0) {
                    sw.set((int)(rnd() & 1));                                          // may bump the epoch
                } else if (op <= 2) {                                                  // the tuner's pin: replace only what nobody uses
                    const Entry e = make_entry(id, 1 + (int)(rnd() % 50), 1);
                    const bool ok = cache.locked([&](auto& m) {
                        auto f = m.find(key);
                        if (f != m.end() && !f->second.tuner_owned) return false;
                        m[key] = e;
                        return true;
                    });
                    (ok ? pins : refused)++;
                } else if (op == 3) {                                                  // commit
                    cache.locked([&](auto& m) {
                        auto f = m.find(key);
                        if (f != m.end()) f->second.tuner_owned = 0;
                    });
                } else {                                                               // a launch: find, else plan outside the lock and insert
                    Entry e;
                    finds++;
                    if (cache.find(key, e, epoch)) {
                        hits++;
                        REQUIRE(whole(e, id));
                        if (!e.tuner_owned) {      // handed out: neither insert nor pin may replace it while the epoch stands
                            Entry again;
                            unsigned epoch2;
                            sw.get(&epoch2);
                            if (cache.find(key, again, epoch) && epoch2 == epoch) REQUIRE(whole(again, id));
                        }
                    } else {
                        cache.insert(key, make_entry(id, 0, 0));
                    }
                }
            }
        });
    for (int t = 0; t < N_THREADS; ++t) th[t].join();
    REQUIRE(finds > 0 && hits > 0 && pins > 0);
    // insert keeps the first entry
    const std::string k0 = plan_key(make_desc(100));
    cache.insert(k0, make_entry(100, 1, 0));
    cache.insert(k0, make_entry(100, 2, 0));
    Entry e;
    unsigned epoch;
    sw.get(&epoch);
    REQUIRE(!cache.find(k0, e, epoch + 1) && !cache.find(k0, e, epoch + 1));      // (the epoch change dropped it)
    cache.insert(k0, make_entry(100, 1, 0));
    cache.insert(k0, make_entry(100, 2, 0));
    REQUIRE(cache.find(k0, e, epoch + 1) && e.version == 1 && whole(e, 100));
    printf("conv_host_check: ok (%ld finds, %ld hits, %ld pins, %ld pins refused)\n", finds.load(), hits.load(), pins.load(), refused.load());
    return 0;
}
