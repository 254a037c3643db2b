// The host layer every convolution file shares: descriptor checks, the plan cache and its key, the "plan every shape" switch, the
// small plan helpers (tile_begin, slab count, vec4 epilogue) and, for files built with hipcc, the slot-table upload, the trace buffer
// and the one launch prologue of kernels with > 64 KB of dynamic LDS.  A new kernel file keeps its own planner and domain
// conditions and takes everything else from here.
//
// The part above the __HIPCC__ block needs no HIP runtime: tools/conv_host_check.cpp builds it with a plain host compiler under the
// thread and address sanitizers.
#pragma once
#include <stdint.h>

#include <initializer_list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#include "common.h"
#else
#include "../../include/radar_depth_hip.h"
namespace rd { void set_error(const char* fmt, ...); }      // (a stand-alone host build supplies its own)
#endif

namespace rd {

// ---- descriptor checks.  The per-kernel domain conditions (channel minima, stride limits, each kernel's 2 GiB formula, planner
// rules) stay in the kernel's file; these are the checks every kernel repeats.
// bool form: phase count in range, every phase non-empty with 1..max_taps taps, every tap inside its declared range
bool desc_taps_ok(const RdConvDesc& d, int max_taps = RD_MAX_TAPS);
// message form (rd_last_error() texts prefixed "<who>: "): null descriptor, phase count, then `domain` (the caller's own conditions,
// which fire before the per-phase ones), then tap count, empty phase and tap range of every phase
int check_desc(const RdConvDesc* d, const char* who, int (*domain)(const RdConvDesc& d));

// ---- the cache key: the descriptor's bytes with the four tile_begin fields zeroed (the library fills them; a caller's stale value
// must not make a second entry), then the tag words
std::string plan_key(const RdConvDesc& d, std::initializer_list<int> tag = {});

// Largest weight-slab index of any tap, plus one
int weight_slabs(const RdConvDesc& d);
// tile_begin of every phase for TH x TW pixel tiles; returns the tile total
int fill_tile_begin(RdConvDesc& d, int TH, int TW);
// the row-tiled form (tiles of BM rows over N * lh * lw): tile_begin[0 .. RD_MAX_PHASES], phases past n_phases hold the total
int fill_row_tile_begin(const RdConvDesc& d, int BM, int (&tile_begin)[RD_MAX_PHASES + 1]);

// The epilogue may move four channels at a time: Cout, the strides and act_cols multiples of 4, out / addend aligned to four channels
// of the storage type (elem_bytes 4 or 2), bias to 16 bytes
static inline bool epilogue_vec4_ok(const void* out, int ldo, int Cout, int act_cols, const void* addend, int ld_add, const float* bias,
                                    int elem_bytes) {
    const uintptr_t al = 4 * (uintptr_t)elem_bytes;
    return Cout % 4 == 0 && ldo % 4 == 0 && reinterpret_cast<uintptr_t>(out) % al == 0 && act_cols % 4 == 0 &&
           (!addend || (ld_add % 4 == 0 && reinterpret_cast<uintptr_t>(addend) % al == 0)) &&
           (!bias || reinterpret_cast<uintptr_t>(bias) % 16 == 0);
}

// ---- "plan every shape the kernel can run" (tests / sweeps): the value, its lazy start from the environment, and an epoch that
// drops the plans cached under the other setting
class PlanAllSwitch {
public:
    explicit PlanAllSwitch(bool (*from_env)()) : from_env_(from_env) {}
    bool get(unsigned* epoch = nullptr) {
        std::lock_guard<std::mutex> lk(mu_);
        if (all_ < 0) all_ = from_env_() ? 1 : 0;
        if (epoch) *epoch = epoch_;
        return all_ == 1;
    }
    int set(int on) {       // returns the previous setting
        std::lock_guard<std::mutex> lk(mu_);
        if (all_ < 0) all_ = from_env_() ? 1 : 0;
        const int prev = all_;
        if ((on != 0) != (prev == 1)) { all_ = on ? 1 : 0; ++epoch_; }
        return prev;
    }
private:
    bool (*from_env_)();
    std::mutex mu_;
    int all_ = -1;          // -1: not set yet (the environment decides at first use)
    unsigned epoch_ = 0;
};

// ---- plans are a pure function of the descriptor: cached, because a step is issued as ~650 plain launches and a tile search (tens
// of microseconds) would otherwise run on every one.  The lock is never held while a planner runs: find, plan outside, insert.  An
// entry handed out is never replaced by insert (the caller may have sized buffers on it).  Whether failures are cached is the
// caller's policy (an Entry with an ok field, or no insert).
template <class Entry>
class PlanCache {
public:
    // copies the entry out under the lock; a changed epoch (PlanAllSwitch) first drops every entry
    bool find(const std::string& key, Entry& out, unsigned epoch = 0) {
        std::lock_guard<std::mutex> lk(mu_);
        if (epoch != epoch_) { map_.clear(); epoch_ = epoch; }
        auto it = map_.find(key);
        if (it == map_.end()) return false;
        out = it->second;
        return true;
    }
    // keeps the first entry of a key
    void insert(std::string key, const Entry& e) {
        std::lock_guard<std::mutex> lk(mu_);
        map_.emplace(std::move(key), e);
    }
    // find-and-modify / replace for the tuner of gconv.hip: f(map) runs under the lock
    template <class F>
    auto locked(F&& f) {
        std::lock_guard<std::mutex> lk(mu_);
        return f(map_);
    }
private:
    std::mutex mu_;
    std::unordered_map<std::string, Entry> map_;
    unsigned epoch_ = 0;
};

#ifdef __HIPCC__
// Slot table of a plan on the current device: hipMalloc + one synchronous copy (a few KB, at the first launch of the plan; never
// freed).  nullptr on failure.
const int* upload_slot_table(const std::vector<int>& host);

// Diagnostics: STAMPS cycle-counter slots for each of up to 65536 workgroups of the last traced launch
template <int STAMPS>
struct TraceBuf {
    unsigned long long* buf = nullptr;
    int get(unsigned long long*& dev) {      // lazy allocation
        if (!buf) RD_CHECK_HIP(hipMalloc(&buf, (size_t)65536 * STAMPS * sizeof(unsigned long long)));
        dev = buf;
        return RD_OK;
    }
    int read(unsigned long long* host, int n_wg) const {
        if (!buf) return RD_EINVAL;
        RD_CHECK_HIP(hipMemcpy(host, buf, (size_t)n_wg * STAMPS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return RD_OK;
    }
};

// The launch prologue of every kernel that may use more than 64 KB of dynamic LDS: raise the kernel's limit to lds_cap once per
// device (AttrOnce, common.h), launch, check.  One attribute bit set per kernel K.
template <auto K, class... Args>
int launch_dyn_lds(const char* name, dim3 grid, dim3 block, size_t lds, size_t lds_cap, hipStream_t s, const Args&... a) {
    static std::atomic<unsigned long long> attr_set{0};
    RD_SET_ATTR_ONCE(attr_set, hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap));
    hipLaunchKernelGGL(K, grid, block, lds, s, a...);
    RD_CHECK_LAUNCH(name);
    return RD_OK;
}
#endif

}  // namespace rd
