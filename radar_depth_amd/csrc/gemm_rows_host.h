// The host half of the two channel-grouped row GEMMs (gemm1_split.hip: one tap per phase; gemm_taps_split.hip: up to four): plan,
// the three queries and the launch.  Each kernel file describes itself in a struct K:
//   Args                        the kernel's argument struct
//   name                        prefix of the error texts
//   CK, MAX_TAPS                input channels per stage, taps per phase
//   enabled()                   A/B switch of the kernel (read once)
//   nt(Cout)                    column tiles of 32 per workgroup
//   lds(BM, BN)                 dynamic LDS bytes of a BM x BN tile
//   marker(d)                   out[7] of plan-info
//   launch<MT, NT>(a, grid, lds, s)
#pragma once
#include "conv_host.h"

namespace rd {

struct RowGemmPlan { int MT, NT, n_cotiles, tiles; int tile_begin[RD_MAX_PHASES + 1]; size_t lds; };

template <class K>
static bool row_gemm_plan(const RdConvDesc* d, RowGemmPlan& pl) {
    if (!K::enabled() || !d || d->n_phases < 1 || d->n_phases > RD_MAX_PHASES) return false;
    if (d->in_stride < 1 || d->in_stride > 2 || d->out_stride < 1 || d->out_stride > 2) return false;
    if (d->Cin % K::CK != 0 || d->Cin < 32 || d->Cout < 32 || d->Cout % 8 != 0 || d->ldi % 4 != 0) return false;
    // (the kernels address `in` in 8-byte units from the tensor base, not per image)
    if ((int64_t)d->N * d->Hi * d->Wi * d->ldi / 2 >= (int64_t)0x80000000u) return false;
    int64_t rows = 0;
    for (int i = 0; i < d->n_phases; ++i) {
        const RdPhase& p = d->phase[i];
        if (p.n_taps < 1 || p.n_taps > K::MAX_TAPS || p.lh < 1 || p.lw < 1) return false;
        for (int t = 0; t < p.n_taps; ++t)
            if (p.widx[t] < 0) return false;
        rows += (int64_t)d->N * p.lh * p.lw;
    }
    pl.NT = K::nt(d->Cout);
    if (d->Cout % (pl.NT * 32) != 0) return false;        // (the weight copies read whole column tiles)
    pl.n_cotiles = d->Cout / (pl.NT * 32);
    // 256-row tiles when they still give every CU its two workgroups, else 128-row tiles
    pl.MT = (rows / 256) * pl.n_cotiles >= 2 * (int64_t)num_cus() ? 2 : 1;
    const int BM = 4 * pl.MT * 32, BN = pl.NT * 32;
    pl.tiles = fill_row_tile_begin(*d, BM, pl.tile_begin);
    pl.lds = K::lds(BM, BN);
    return pl.lds <= 80 * 1024 - 256;
}

template <class K>
static int row_gemm_supported(const RdConvDesc* d) {
    RowGemmPlan pl;
    return row_gemm_plan<K>(d, pl) ? 1 : 0;
}

template <class K>
static int row_gemm_stat_tiles(const RdConvDesc* d) {
    RowGemmPlan pl;
    return row_gemm_plan<K>(d, pl) ? pl.tiles : RD_EINVAL;
}

// diagnostics: out[0..7] = MT, NT, rows per tile, 1, 0, LDS bytes, workgroups, K::marker
template <class K>
static int row_gemm_plan_info(const RdConvDesc* d, int32_t* out) {
    RowGemmPlan pl;
    if (!out || !row_gemm_plan<K>(d, pl)) return RD_EINVAL;
    const int v[8] = {pl.MT, pl.NT, 4 * pl.MT * 32, 1, 0, (int)pl.lds, pl.tiles * pl.n_cotiles, K::marker(*d)};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return RD_OK;
}

template <class K>
static int row_gemm_launch(const RdConvDesc* d, const float* in, const void* w_split, int64_t piece_elems, float* out, const float* bias, int32_t act,
                           int32_t act_cols, const float* addend, int32_t ld_add, float* stat_partial, hipStream_t s) {
    typename K::Args a;
    RowGemmPlan pl;
    if (!row_gemm_plan<K>(d, pl)) { set_error("%s: descriptor not supported", K::name); return RD_EINVAL; }
    RD_CHECK_ARG(in && w_split && out, "%s: null argument", K::name);
    RD_CHECK_ARG(reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(w_split) % 16 == 0, "%s: unaligned tensor", K::name);
    RD_CHECK_ARG(piece_elems >= (int64_t)weight_slabs(*d) * d->Cin * d->Cout && piece_elems % 8 == 0, "%s: piece stride %lld too small", K::name,
                 (long long)piece_elems);
    a.d = *d;
    a.in = in; a.w = static_cast<const unsigned short*>(w_split); a.out = out; a.addend = addend; a.bias = bias; a.stat = stat_partial;
    a.act = act; a.act_cols = act_cols; a.ld_add = ld_add; a.ldw = d->Cout;
    a.n_cotiles = pl.n_cotiles;
    a.wplane = (long long)piece_elems * 2;
    a.vec4 = epilogue_vec4_ok(out, d->ldo, d->Cout, act_cols, addend, ld_add, bias, 4);
    for (int i = 0; i <= RD_MAX_PHASES; ++i) a.tile_begin[i] = pl.tile_begin[i];
    const int grid = pl.tiles * pl.n_cotiles;
    if (pl.MT == 2 && pl.NT == 2) return K::template launch<2, 2>(a, grid, pl.lds, s);
    if (pl.MT == 1 && pl.NT == 2) return K::template launch<1, 2>(a, grid, pl.lds, s);
    if (pl.MT == 2 && pl.NT == 1) return K::template launch<2, 1>(a, grid, pl.lds, s);
    return K::template launch<1, 1>(a, grid, pl.lds, s);
}

}  // namespace rd
