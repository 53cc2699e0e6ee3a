// The unit body of the logit kernels, shared by cpn_local_units (local_units.hip: the stand-alone kernel, one logit per row to
// global memory) and cpn_attend_units (attend_units.hip: the same logits handed to the hidden sum through LDS).  Both
// instantiate THESE device functions, so a unit's accumulators receive the same instructions in the same order whichever kernel
// runs it: the two produce the same bits by construction, and stay doing so.  What differs between them is outside the unit:
// which units a wave walks (Seq), where a row's dot product goes (Sink) and what happens between two units (the fused kernel's
// barrier, taken inside Seq::after).
// Layouts, the three modes and the structure of the body: local_units.hip.
#pragma once
#include "encode_common.h"

// timing-only ablations of the STAND-ALONE kernel (tools/lu_check.py; results are wrong when non-zero): 1 = the other operand
// (kh / ce fragments) is not loaded, 2 = no `add` rows, 4 = the per-row inputs are fetched once (no loads inside the loop),
// 8 = no stores (the sink's business), 16 = no 128 -> 128 layers (their LDS reads and MFMAs)
#ifndef CPN_LU_ABLATE
#define CPN_LU_ABLATE 0
#endif

namespace {

struct UnitGeo {
    int V, R, S, ray0, nrays, nsblk, groups_per_b;
    long long group0, nunits;
};

// the ray groups (TG adjacent rays of one batch element) a call's ray range touches, partial ones included
__host__ inline UnitGeo unit_geo(int V, int R, int S, int ray0, int nrays) {
    UnitGeo geo;
    geo.V = V; geo.R = R; geo.S = S; geo.ray0 = ray0; geo.nrays = nrays;
    geo.nsblk = (int)cpn_cdiv(S, TSW);
    geo.groups_per_b = (int)cpn_cdiv(R, TG);
    const int b_lo = ray0 / R, b_hi = (ray0 + nrays - 1) / R;
    geo.group0 = (long long)b_lo * geo.groups_per_b + (ray0 - b_lo * R) / TG;
    const long long group1 = (long long)b_hi * geo.groups_per_b + (ray0 + nrays - 1 - b_hi * R) / TG;
    geo.nunits = (group1 - geo.group0 + 1) * V * geo.nsblk;
    return geo;
}

// the global operands of the body (cpn_local_units' arguments)
struct UnitArgs {
    const float* loc8; const float* coords9;
    const float* w1; int ldw1; const float* b1; const float* add;
    const __half* w2; int ldw2; const float* b2;
    const __half* wk2; int ldwk2; const float* bk2;
    const float* w1b; int ldw1b; const float* b1b;
    const __half* kh_u; __half* ce_u; const f32x4* lv_u;
};

// the workgroup's LDS copy of the weights: layer-2 fragments [tile t][k block p][lane], biases, first-layer A fragments
// [set][tile][lane] (sets: hi, lo (, query_embed's hi, lo in mode 2))
struct UnitLds {
    half8* w2l; half8* wkl; float* b2s; float* bks; half4* w1s;
};
template <int MODE>
__host__ __device__ constexpr size_t unit_lds_bytes() {
    return (size_t)(MODE != 1 ? 2 : 1) * 8 * 4 * 64 * sizeof(half8) + 2 * 128 * sizeof(float) + (size_t)(MODE == 2 ? 4 : 2) * 8 * 64 * sizeof(half4);
}

// MODE 2: (w1, b1, add, w2, b2) are the round-2 query layers as in mode 1; (w1b, b1b) = query_embed, (wk2, bk2) = query_embed_2
// two accumulator tiles (channels 8 fg .. + 4 and + 4 .. + 8 of a 32-block) -> one fp16 B-operand / fragment register quad, as
// PACKED conversions (v_cvt_pk_f16_f32, round to nearest even) and a packed ReLU behind the rounding (the same value as rounding
// behind the ReLU: rounding is monotone and keeps the sign) - written element by element the compiler emitted a v_max_f32, a
// v_cvt_f16_f32 and half a v_perm_b32 per value, and the kernel's SIMDs were issue-bound (VALU 51 % + MFMA 44 % of their cycles)
template <bool RELU>
__device__ __forceinline__ half8 pack_tiles(const f32x4& lo, const f32x4& hi) {
    half8 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4& src = q < 2 ? lo : hi;
        const f32x2v two = {src[2 * (q & 1)], src[2 * (q & 1) + 1]};
        half2v hv = __builtin_convertvector(two, half2v);
        if (RELU) hv = __builtin_elementwise_max(hv, (half2v){(_Float16)0.0f, (_Float16)0.0f});
        out[2 * q] = hv[0];
        out[2 * q + 1] = hv[1];
    }
    return out;
}

// Stage the weights in LDS: `nthreads` threads (tid = 0 .. nthreads - 1, whole waves) share the copy, the wave tid < 64 splits
// the first layers.  The caller synchronises the workgroup before the first unit.
template <int MODE>
__device__ __forceinline__ void unit_stage_weights(const UnitLds& L, const UnitArgs& A, int tid, int nthreads) {
    const int lane = tid & 63;
    const int a = lane & 15, fg = lane >> 4;
    for (int i = tid; i < 8 * 4 * 64; i += nthreads) {
        const int l = i & 63, p = (i >> 6) & 3, t = i >> 8;
        const int ch = (t >> 1) * 32 + ((l & 15) >> 2) * 8 + (t & 1) * 4 + (l & 3);       // output channel of tile row
        L.w2l[i] = *reinterpret_cast<const half8*>(A.w2 + (size_t)ch * A.ldw2 + p * 32 + (l >> 4) * 8);
        if constexpr (MODE != 1) L.wkl[i] = *reinterpret_cast<const half8*>(A.wk2 + (size_t)ch * A.ldwk2 + p * 32 + (l >> 4) * 8);
    }
    if (tid < 128) {
        L.b2s[tid] = A.b2[tid];
        L.bks[tid] = MODE != 1 ? A.bk2[tid] : 0.0f;
    }
    // First layer (K = 16, fp32 weights and inputs) on the fp16 MFMA as a hi / lo split - w = wh + wl, x = xh + xl (each part
    // an fp16), w . x = wh xh + wh xl + wl xh up to 2^-22 |w x| - three v_mfma_f32_16x16x16_f16 of 8 cycles per tile instead
    // of four v_mfma_f32_16x16x4_f32 of 32: the fp32 MFMA runs at 1/16 of the fp16 rate and was two thirds of this
    // kernel's matrix time (cpn_local_mlp keeps the fp32 form).
    // (the A fragments live in LDS and are read where they are used: held in registers they were 32 (64) of the 128 a wave
    // may have at four waves per SIMD)
    if (tid < 64) {
        auto split = [&](const float* wsrc, int ldw, const float* bsrc, int ch, half4& hi, half4& lo) {
            f32x4 wv = *reinterpret_cast<const f32x4*>(wsrc + (size_t)ch * ldw + fg * 4);
            if (fg == 0) wv[3] = bsrc[ch];                     // K slot 3 is unused by the inputs: bias x 1.0
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                hi[i] = (_Float16)wv[i];
                lo[i] = (_Float16)(wv[i] - (float)hi[i]);
            }
        };
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int ch = (t >> 1) * 32 + (a >> 2) * 8 + (t & 1) * 4 + (a & 3);
            half4 hi, lo;
            split(A.w1, A.ldw1, A.b1, ch, hi, lo);
            L.w1s[(0 * 8 + t) * 64 + lane] = hi;
            L.w1s[(1 * 8 + t) * 64 + lane] = lo;
            if constexpr (MODE == 2) {
                split(A.w1b, A.ldw1b, A.b1b, ch, hi, lo);
                L.w1s[(2 * 8 + t) * 64 + lane] = hi;
                L.w1s[(3 * 8 + t) * 64 + lane] = lo;
            }
        }
    }
}

// The units of one wave, U at a time.
//   Seq:  niter()                 iterations of this wave (every wave of a workgroup that takes barriers in after() must see the
//                                 trip count its workgroup agreed on)
//         unit(it, u, live)       the u-th unit of iteration `it`, relative to geo.group0; a unit that does not exist is some unit
//                                 that does (walked again, live = false: nothing of it is stored).  `it` may be niter() (the
//                                 look-ahead of the last iteration).
//         after(it)               end of iteration `it`, behind its sink calls
//   Sink: sink(it, u, srow, d)    called by every lane: d = the logit of this lane's row (a = lane & 15; all four fg hold it),
//                                 srow = its row in row order, ((ray - ray0) * V + v) * S + s, or -1 for a row that is dead
template <int MODE, int U, class Seq, class Sink>
__device__ __forceinline__ void unit_walk(const UnitLds& L, const UnitArgs& A, const UnitGeo& geo, const int lane, Seq& seq,
                                          Sink& sink) {
    const int a = lane & 15, fg = lane >> 4;
    const int V = geo.V, R = geo.R, S = geo.S;
    const float* __restrict__ loc8 = A.loc8;
    const float* __restrict__ coords9 = A.coords9;
    const float* __restrict__ add = A.add;
    const __half* __restrict__ kh_u = A.kh_u;
    __half* __restrict__ ce_u = A.ce_u;
    const f32x4* __restrict__ lv_u = A.lv_u;

    struct RowIn {
        f32x4 lv;          // this lane's 4 K entries of the 16-wide input
        unsigned rayrel;   // ray - ray0 (row of `add`)
        long long srow;    // row of the (rows, .) arrays in row order; -1: dead row of the unit
    };
    // row c of unit uu: the map of encode_fused.hip (uu = ((ray group - group0) * V + v) * nsblk + sample block)
    auto fetch = [&](unsigned uu) {
        const int sblk = (int)(uu % (unsigned)geo.nsblk);
        const int v = (int)((uu / (unsigned)geo.nsblk) % (unsigned)V);
        const long long gq = geo.group0 + uu / ((unsigned)geo.nsblk * (unsigned)V);
        const int b = (int)(gq / geo.groups_per_b), rgroup = (int)(gq % geo.groups_per_b);
        const RowId id = tile_row(a, rgroup, sblk, S, R, b, geo.ray0, geo.nrays);
        const int r = min(id.r, R - 1), s = min(id.s, S - 1);
        const size_t nr = ((size_t)(b * V + v)) * R + r;
        const float* lp = loc8 + (nr * S + s) * 8;
        const float* c9 = coords9 + nr * 9;
        RowIn o;
        const long long rayrel = (long long)b * R + r - geo.ray0;
        o.rayrel = (unsigned)max(0LL, min(rayrel, (long long)geo.nrays - 1));
        o.srow = id.live ? (rayrel * V + v) * S + s : -1;
        if (lv_u) {
            // the lane's four inputs as cpn_sample_geometry packed them: ONE coalesced 1 KiB read per unit instead of five
            // scattered ones (3 - 16 bytes per lane from 16 rows and 4 rays: 0.26 of mode 0's 0.9 ms, 0.5 of mode 2's 1.2 ms,
            // tools/lu_check.py).  Rows that do not exist (R or S no multiple of 4) hold whatever the buffer held: their
            // MFMA columns are their own and nothing of them is stored
            o.lv = __builtin_nontemporal_load(lv_u + (size_t)uu * 64 + lane);
            return o;
        }
        if (fg == 0) { const f32x4 l0 = *reinterpret_cast<const f32x4*>(lp); o.lv = f32x4{l0[0], l0[1], l0[2], 1.0f}; }
        else if (fg == 1) o.lv = f32x4{0.f, 0.f, c9[0], c9[1]};
        else if (fg == 2) o.lv = f32x4{c9[2], lp[3], lp[4], lp[5]};
        else o.lv = f32x4{lp[6], c9[6], c9[7], c9[8]};
        return o;
    };

    // A 128 -> 128 layer on the wave's U units: o[u][t] = bias + sum_p W(t, p) . b[u][p].  The 32 fragments are read from LDS FD
    // ahead of the MFMAs that use them, k block outer (two MFMAs on one accumulator are 8 U instructions apart), and every
    // fragment is multiplied against ALL the wave's units: with one unit per wave the 1 KiB fragment read (4 clocks of the CU's
    // one LDS pipe) feeds a single 16-clock MFMA, and four SIMDs asking for one each saturate that pipe exactly when the matrix
    // cores would (measured floor with no global loads at all: 0.55 / 0.67 ms for 0.26 / 0.30 ms of MFMA).  Each accumulator
    // still receives bias, p = 0, 1, 2, 3 in that order: the results do not change.
    auto layer128 = [&](const half8* wfr, const float* bias_s, const half8 (&b)[U][4], f32x4 (&o)[U][8]) {
        constexpr int NF = 32, FD = 4;
        if (CPN_LU_ABLATE & 16) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int t = 0; t < 8; ++t) o[u][t] = f32x4{b[u][t & 3][0], b[u][t & 3][1], b[u][t & 3][2], b[u][t & 3][3]};
            return;
        }
        half8 af[FD];
#pragma unroll
        for (int d = 0; d < FD; ++d) af[d] = wfr[(((d & 7) * 4) + (d >> 3)) * 64 + lane];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_s + (t >> 1) * 32 + fg * 8 + (t & 1) * 4);
#pragma unroll
            for (int u = 0; u < U; ++u) o[u][t] = bv;
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int t = i & 7, pblk = i >> 3;
#pragma unroll
            for (int u = 0; u < U; ++u) o[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i % FD], b[u][pblk], o[u][t], 0, 0, 0);
            if (i + FD < NF) af[i % FD] = wfr[((((i + FD) & 7) * 4) + ((i + FD) >> 3)) * 64 + lane];
        }
        __builtin_amdgcn_sched_group_barrier(0x100, FD + 8, 0);      // the first FD fragments + the 8 bias reads
#pragma unroll
        for (int i = 0; i < NF - FD; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, U, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, FD * U, 0);
    };
    // the first layer (K = 16 as three hi / lo MFMAs per tile) of set `ws` (0: w1 / b1, 2: w1b / b1b) on the U units
    auto layer16 = [&](int ws, const half4 (&xh)[U], const half4 (&xl)[U], f32x4 (&o)[U][8]) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const half4 wh = L.w1s[(ws * 8 + t) * 64 + lane], wl = L.w1s[((ws + 1) * 8 + t) * 64 + lane];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                o[u][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(wl, xh[u], o[u][t], 0, 0, 0);
                o[u][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(wh, xl[u], o[u][t], 0, 0, 0);
                o[u][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(wh, xh[u], o[u][t], 0, 0, 0);
            }
        }
    };
    auto add_rows = [&](unsigned rayrel, f32x4 (&dst)[8]) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
            dst[t] = (CPN_LU_ABLATE & 2) ? f32x4{0.f, 0.f, 0.f, 0.f}
                                         : *reinterpret_cast<const f32x4*>(add + (size_t)rayrel * 128 + (t >> 1) * 32 + fg * 8 + (t & 1) * 4);
    };

    const unsigned niter = seq.niter();
    if (niter == 0) return;
    RowIn cur[U];
    constexpr bool ADD_AHEAD = MODE == 2 && U == 1;            // (two units per wave leave no registers for it, and need it less)
    f32x4 addn[ADD_AHEAD ? U : 1][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        bool l0;
        cur[u] = fetch(seq.unit(0u, u, l0));
        if constexpr (ADD_AHEAD) add_rows(cur[u].rayrel, addn[u]);
    }
    for (unsigned it = 0; it < niter; ++it) {
        RowIn nxt[U];
        unsigned un[U];
        bool ulive[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bool ln;
            un[u] = seq.unit(it, u, ulive[u]);
            nxt[u] = (CPN_LU_ABLATE & 4) ? cur[u] : fetch(seq.unit(it + 1, u, ln));
        }
        // the other operand of the dot product, as B fragments / accumulator-layout rows: 4 x 1 KiB of contiguous memory
        // (requesting it a unit ahead was measured: no change - the kernel is not waiting for it)
        half8 cv[U][4];
        if constexpr (MODE != 2) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    cv[u][p] = (CPN_LU_ABLATE & 1) ? half8{} : __builtin_nontemporal_load(
                        reinterpret_cast<const half8*>(MODE == 0 ? kh_u : ce_u) + ((size_t)un[u] * 4 + p) * 64 + lane);
        }
        f32x4 acc[U][8];
        half4 xh[U], xl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (ADD_AHEAD) {
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[u][t] = addn[u][t];        // requested an iteration ahead (1.17 -> 0.91 ms)
                add_rows(nxt[u].rayrel, addn[u]);
            } else if constexpr (MODE != 0) {
                add_rows(cur[u].rayrel, acc[u]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xh[u][i] = (_Float16)cur[u].lv[i];
                xl[u][i] = (_Float16)(cur[u].lv[i] - (float)xh[u][i]);
            }
        }
        if constexpr (MODE == 2) {
            // coords_embed of these units, exactly as mode 0 forms it (same instructions, same order: the bits mode 0 would have stored)
            f32x4 ab[U][8];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int t = 0; t < 8; ++t) ab[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            layer16(2, xh, xl, ab);
            half8 hq[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p) hq[u][p] = pack_tiles<true>(ab[u][2 * p], ab[u][2 * p + 1]);
            f32x4 oq[U][8];
            layer128(L.wkl, L.bks, hq, oq);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p) cv[u][p] = pack_tiles<false>(oq[u][2 * p], oq[u][2 * p + 1]);
        }
        layer16(0, xh, xl, acc);
        // hidden layer -> fp16 B operands: K block p = channels p*32 .. p*32+31, this lane holds fg*8 .. fg*8+7 of it
        half8 hb[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int p = 0; p < 4; ++p) hb[u][p] = pack_tiles<true>(acc[u][2 * p], acc[u][2 * p + 1]);
        f32x4 o2[U][8];
        layer128(L.w2l, L.b2s, hb, o2);
        long long srow[U];
        float dsum[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            srow[u] = ulive[u] ? cur[u].srow : -1;
            cur[u] = nxt[u];
            dsum[u] = 0.0f;
        }
        if constexpr (MODE == 0) {
            // coords_embed leaves in unit order as it is (the accumulator layout is the fragment layout), and meets the key:
            // key_map_2 on the B fragments of kh, in the same accumulator layout
            half8 ce[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    ce[u][p] = pack_tiles<false>(o2[u][2 * p], o2[u][2 * p + 1]);
                    if (ce_u && ulive[u] && !(CPN_LU_ABLATE & 8))                     // NULL: round 2 recomputes it (mode 2)
                        reinterpret_cast<half8*>(ce_u)[((size_t)un[u] * 4 + p) * 64 + lane] = ce[u][p];
                }
            f32x4 k2[U][8];
            layer128(L.wkl, L.bks, cv, k2);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const half8 kp = pack_tiles<false>(k2[u][2 * p], k2[u][2 * p + 1]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) dsum[u] += (float)kp[e] * (float)ce[u][p][e];
                }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const half8 qp = pack_tiles<false>(o2[u][2 * p], o2[u][2 * p + 1]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dsum[u] += (float)qp[i] * (float)cv[u][p][i];
                        dsum[u] += (float)qp[4 + i] * (float)cv[u][p][4 + i];
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float d = dsum[u];
            d += __shfl_xor(d, 16);
            d += __shfl_xor(d, 32);
            sink(it, u, srow[u], d);
        }
        seq.after(it);
    }
}

}  // namespace
