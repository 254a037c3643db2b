// The non-template half of conv_host.h.
#include "conv_host.h"

#include <stddef.h>
#include <string.h>

namespace rd {

bool desc_taps_ok(const RdConvDesc& d, int max_taps) {
    if (d.n_phases < 1 || d.n_phases > RD_MAX_PHASES) return false;
    for (int i = 0; i < d.n_phases; ++i) {
        const RdPhase& p = d.phase[i];
        if (p.n_taps < 1 || p.n_taps > max_taps || p.lh < 1 || p.lw < 1) return false;
        for (int t = 0; t < p.n_taps; ++t)
            if (p.dh[t] < p.dh_min || p.dh[t] > p.dh_max || p.dw[t] < p.dw_min || p.dw[t] > p.dw_max) return false;
    }
    return true;
}

#define RD_CHECK_DESC(cond, ...)            \
    do {                                    \
        if (!(cond)) {                      \
            set_error(__VA_ARGS__);         \
            return RD_EINVAL;               \
        }                                   \
    } while (0)

int check_desc(const RdConvDesc* d, const char* who, int (*domain)(const RdConvDesc& d)) {
    RD_CHECK_DESC(d != nullptr, "%s: null descriptor", who);
    RD_CHECK_DESC(d->n_phases >= 1 && d->n_phases <= RD_MAX_PHASES, "%s: n_phases=%d", who, d->n_phases);
    const int rc = domain(*d);
    if (rc != RD_OK) return rc;
    for (int i = 0; i < d->n_phases; ++i) {
        const RdPhase& p = d->phase[i];
        RD_CHECK_DESC(p.n_taps >= 1 && p.n_taps <= RD_MAX_TAPS, "%s: phase %d has %d taps", who, i, p.n_taps);
        RD_CHECK_DESC(p.lh >= 1 && p.lw >= 1, "%s: empty phase %d", who, i);
        for (int t = 0; t < p.n_taps; ++t)
            RD_CHECK_DESC(p.dh[t] >= p.dh_min && p.dh[t] <= p.dh_max && p.dw[t] >= p.dw_min && p.dw[t] <= p.dw_max,
                          "%s: tap %d of phase %d outside its declared range", who, t, i);
    }
    return RD_OK;
}
#undef RD_CHECK_DESC

std::string plan_key(const RdConvDesc& d, std::initializer_list<int> tag) {
    std::string key;
    key.reserve(sizeof(RdConvDesc) + tag.size() * sizeof(int));      // (one allocation, one copy: built at every launch)
    key.assign(reinterpret_cast<const char*>(&d), sizeof(RdConvDesc));
    for (int i = 0; i < RD_MAX_PHASES; ++i)
        memset(&key[offsetof(RdConvDesc, phase) + i * sizeof(RdPhase) + offsetof(RdPhase, tile_begin)], 0, sizeof(int32_t));
    for (int t : tag) key.append(reinterpret_cast<const char*>(&t), sizeof(int));
    return key;
}

int weight_slabs(const RdConvDesc& d) {
    int S = 0;
    for (int i = 0; i < d.n_phases; ++i)
        for (int t = 0; t < d.phase[i].n_taps; ++t) S = S > d.phase[i].widx[t] + 1 ? S : d.phase[i].widx[t] + 1;
    return S;
}

int fill_tile_begin(RdConvDesc& d, int TH, int TW) {
    int tb = 0;
    for (int i = 0; i < d.n_phases; ++i) {
        d.phase[i].tile_begin = tb;
        tb += ((d.phase[i].lh + TH - 1) / TH) * ((d.phase[i].lw + TW - 1) / TW);
    }
    return tb;
}

int fill_row_tile_begin(const RdConvDesc& d, int BM, int (&tile_begin)[RD_MAX_PHASES + 1]) {
    int tb = 0;
    for (int i = 0; i < d.n_phases; ++i) {
        tile_begin[i] = tb;
        tb += (int)(((int64_t)d.N * d.phase[i].lh * d.phase[i].lw + BM - 1) / BM);
    }
    for (int i = d.n_phases; i <= RD_MAX_PHASES; ++i) tile_begin[i] = tb;
    return tb;
}

#ifdef __HIPCC__
const int* upload_slot_table(const std::vector<int>& host) {
    int* devp = nullptr;
    if (hipMalloc(&devp, host.size() * sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemcpy(devp, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(devp); return nullptr; }
    return devp;
}
#endif

}  // namespace rd
