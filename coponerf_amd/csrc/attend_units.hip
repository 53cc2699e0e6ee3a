// One attention round in ONE launch (round 7): the logits of cpn_local_units (mode 0 / 2) and the joint softmax + hidden sum of
// cpn_attend_hidden, for the same rays, with the logit arithmetic of one ray group running under the `hid` stream of another.
//   Replaces models/CoPoNeRF.py:408, 446, 450-461 (round 1) and :472-485 (round 2) of the reference.
// Why: the two kernels are complementary - the logits use the matrix cores, the VALU and 66 - 82 KiB of LDS and next to no HBM,
// the sum uses HBM and nothing else - and as two persistent launches they cannot overlap (each fills every CU).
//
// Work item = a RAY GROUP, the TG = 4 adjacent rays cpn_encode_key's unit order groups: V * ceil(S / 4) units of 16 rows, whose
// logits are the 4 x V*S softmax inputs of exactly those rays.  A workgroup owns the groups bid, bid + grid, ... and is
// wave-specialised (the role branch is wave-uniform):
//   NL logit waves   run the unit body of local_units_body.h (the SAME device functions cpn_local_units instantiates: the same
//                    bits), one unit per wave and iteration, and put each live row's dot product into an LDS ring slot
//                    [slot][ray in group][v * S + s] - one group AHEAD of the streaming waves.
//   8 streaming waves, two per ray: each forms the ray's softmax from the slot (both waves of a ray compute the same numbers,
//                    reading the slot only, and write the same weights - there is no barrier narrower than the workgroup),
//                    then streams the ray's T rows of hid for its half of the 208 16-byte column chunks (2 per lane) with
//                    non-temporal loads, up to 2 RU rows per chunk in flight, rows in ascending order into fp32 accumulators.
// Hand-over: ONE s_barrier per ray group that both roles take.  Behind the group's barrier the logit waves fill slot (g + 1) & 1
// while the streaming waves read slot g & 1; the streaming waves' first loads of a group are issued before its barrier, behind the
// last rows of the group before.  There is
// no cross-workgroup flag, no atomic, nothing a workgroup can wait for but its own waves; both roles derive the number of
// barriers from the workgroup's own group count.
// Bit identity with the pair (tests/test_gpu_attend_units.py): logits by construction (shared body); softmax: max is order
// independent, the sum of exponentials reproduces attend_hidden_ray's tree (thread t of 256 adds rows t, t + 256, ..; a 64-lane
// xor butterfly per wave; (w0 + w1) + (w2 + w3)) with lane l standing for threads l, 64 + l, 128 + l, 192 + l; the weighted sum
// adds a ray's rows in ascending order per channel, never split across waves.
#include <algorithm>

#include "hid_sum.h"
#include "local_units_body.h"

namespace {

constexpr int HC = 1664;                 // hidden channels per row [h_own ; h_other]
constexpr int NCHUNK = HC / 8;           // 208 16-byte column chunks
constexpr int NL = 4;                    // logit waves
constexpr int NS = 2 * TG;               // streaming waves: two per ray of the group
constexpr int AU_THREADS = (NL + NS) * 64;
constexpr int RU = HID_BLOCK_ROWS;       // rows per load block (= the blocks of hid_sum.h); up to two blocks in flight per lane and chunk
constexpr int LDS_MAX = 160 * 1024;

// the workgroup barrier of a ray group: LDS writes done, nothing else waited for (global loads stay in flight across it)
__device__ __forceinline__ void group_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// the units of logit wave lw: those of the workgroup's own groups, unit lw + m * NL of each; upw iterations per group for every
// wave (a unit past the group's last is walked as its last, nothing stored), the group's barrier behind the last of them
struct GroupUnits {
    unsigned lw, upg, upw, nmy, bid, nwg;
    __device__ __forceinline__ unsigned niter() const { return nmy * upw; }
    __device__ __forceinline__ unsigned unit(unsigned it, int, bool& live) const {
        it = min(it, nmy * upw - 1);
        const unsigned k = it / upw, idx = lw + (it - k * upw) * NL;
        live = idx < upg;
        return (bid + k * nwg) * upg + min(idx, upg - 1);
    }
    __device__ __forceinline__ void after(unsigned it) const {
        if ((it + 1) % upw == 0) group_barrier();
    }
};
// a row's logit -> its ring slot (and the caller's logits array, when it wants them: precision = "auto")
struct RingLogits {
    float* ring;                         // 2 slots of TG * T floats
    float* __restrict__ logits;
    unsigned lw, upw, nsblk;
    int S, T, a, fg;
    __device__ __forceinline__ void operator()(unsigned it, int, long long srow, float d) const {
        if (srow < 0 || fg != 0) return;
        const unsigned k = it / upw, idx = lw + (it - k * upw) * NL;
        const int v = (int)(idx / nsblk), s = (int)(idx % nsblk) * TSW + (a >> 2);
        ring[(k & 1) * (TG * T) + (a & 3) * T + v * S + s] = d;
        if (logits) logits[srow] = d;
    }
};

template <int MODE>
__global__ __launch_bounds__(AU_THREADS, 3) void attend_units_kernel(UnitArgs args, UnitGeo geo, const __half* __restrict__ hid,
                                                                     __half* __restrict__ hbar, float* __restrict__ at_wt,
                                                                     float* __restrict__ logits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr size_t WB = 8 * 4 * 64 * sizeof(half8);
    UnitLds L;
    L.w2l = reinterpret_cast<half8*>(smem);
    L.wkl = reinterpret_cast<half8*>(smem + WB);
    L.b2s = reinterpret_cast<float*>(smem + 2 * WB);
    L.bks = L.b2s + 128;
    L.w1s = reinterpret_cast<half4*>(L.bks + 128);
    const int V = geo.V, R = geo.R, S = geo.S, T = V * S;
    float* ring = reinterpret_cast<float*>(smem + unit_lds_bytes<MODE>());
    float* wbuf = ring + 2 * TG * T;     // the normalised weights of the group being streamed, [ray in group][row]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    unit_stage_weights<MODE>(L, args, (int)threadIdx.x, AU_THREADS);
    __syncthreads();

    const unsigned upg = (unsigned)(V * geo.nsblk);
    const unsigned ngroups = (unsigned)geo.nunits / upg;
    const unsigned bid = blockIdx.x, nwg = gridDim.x;
    const unsigned nmy = (ngroups - bid + nwg - 1) / nwg;      // the host launches at most `ngroups` workgroups: >= 1

    if (wave < NL) {
        const unsigned upw = (upg + NL - 1) / NL;
        GroupUnits seq{(unsigned)wave, upg, upw, nmy, bid, nwg};
        RingLogits sink{ring, logits, (unsigned)wave, upw, (unsigned)geo.nsblk, S, T, lane & 15, lane >> 4};
        unit_walk<MODE, 1>(L, args, geo, lane, seq, sink);
        return;
    }

    // ---- streaming waves: the issue slot goes to them first - a few VALU instructions per 16-byte load, and the loads they
    // issue are what the kernel's time is made of
    __builtin_amdgcn_s_setprio(1);
    const int sw = wave - NL, j = sw >> 1, half = sw & 1;
    constexpr int CPW = NCHUNK / 2;                            // 104 chunks per wave: lanes 0 .. 63, and 64 + (0 .. 39)
    const int c0 = half * CPW + lane, c1 = half * CPW + min(64 + lane, CPW - 1);
    const bool live1 = lane < CPW - 64;
    const unsigned off0 = (unsigned)c0 * 8, off1 = (unsigned)c1 * 8;          // this lane's two chunks inside a row, in elements
    // The stream is ONE pipeline over the workgroup's groups: the loads run in pairs of RU-row blocks, a0/a1 and b0/b1, and the
    // first block of the NEXT group's ray is issued in front of the last consume of this one - so the wave has RU rows per
    // chunk in flight across the store, the barrier and the softmax as well (with the pipeline restarted per group, all eight
    // waves of the CU sat with nothing in flight for a memory latency once per group).  Rows behind the last whole pair (T not a
    // multiple of 2 RU) are loaded one at a time.
    const int npair = T / (2 * RU);
    struct Ray {
        bool live;                       // a dead ray of a partial group: nothing read or stored
        int b, r;
        size_t lray;
        const __half* hp;                // the ray's rows of hid: wave-uniform (the loads take it as their scalar base)
    };
    auto ray_of = [&](unsigned k) {
        Ray o;
        const long long gq = geo.group0 + bid + (long long)k * nwg;
        o.b = (int)(gq / geo.groups_per_b);
        o.r = (int)(gq % geo.groups_per_b) * TG + j;
        const long long rayrel = (long long)o.b * R + o.r - geo.ray0;
        o.live = k < nmy && o.r < R && rayrel >= 0 && rayrel < geo.nrays;
        o.lray = (size_t)max(0LL, min(rayrel, (long long)geo.nrays - 1));
        o.hp = hid + o.lray * T * HC;
        return o;
    };
    auto issue = [&](const Ray& ray, half8 (&h0)[RU], half8 (&h1)[RU], int row) {
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const __half* rp = ray.hp + (size_t)(row + u) * HC;
            h0[u] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(rp + off0));
            h1[u] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(rp + off1));
        }
    };
    // asks for issue / consume in the order written.  The compiler honours it only in part: it still gathers the loads of both
    // blocks of an iteration in front of its consumes (loads from const __restrict__ memory cross a memory clobber), so a lane
    // has 0 .. 2 RU rows per chunk in flight rather than RU .. 2 RU; this is the form that was measured (HISTORY.md, round 7)
    auto pin = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    half8 a0[RU], a1[RU], b0[RU], b1[RU];
    Ray nxt = ray_of(0);
    if (nxt.live && npair > 0) issue(nxt, a0, a1, 0);
    for (unsigned k = 0; k < nmy; ++k) {
        const Ray ray = nxt;
        nxt = ray_of(k + 1);
        const bool pre = nxt.live && npair > 0;
        const int b = ray.b, r = ray.r;
        group_barrier();
        if (!ray.live) {
            if (pre) issue(nxt, a0, a1, 0);
            continue;
        }

        const float* lg = ring + (k & 1) * (TG * T) + j * T;
        float* wt = wbuf + j * T;
        float lmax = -INFINITY;
        for (int row = lane; row < T; row += 64) lmax = fmaxf(lmax, lg[row] / 11.31f);
        const float gmax = wave_max(lmax);
        float ps[4] = {0.f, 0.f, 0.f, 0.f};                    // partial sums of threads lane, 64 + lane, 128 + lane, 192 + lane
        for (int base = 0; base < T; base += 256) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = base + q * 64 + lane;
                if (row < T) ps[q] += __expf(lg[row] / 11.31f - gmax);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) ps[q] = wave_sum(ps[q]);
        const float inv = 1.0f / ((ps[0] + ps[1]) + (ps[2] + ps[3]));
        for (int row = lane; row < T; row += 64) {
            const float w = __expf(lg[row] / 11.31f - gmax) * inv;
            wt[row] = w;
            if (at_wt && half == 0) {
                const int v = row / S, s = row - v * S;
                at_wt[sample_index(b, V, v, R, r, S, s)] = w;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's weights are in LDS before any lane reads another's

        float acc0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, acc1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto consume = [&](const half8 (&h0)[RU], const half8 (&h1)[RU], int row) {
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const float w = wt[row + u];
                hid_row_acc<true>(acc0, w, h0[u]);             // (the rounding of cpn_attend_hidden's four-row blocks: hid_sum.h)
                hid_row_acc<true>(acc1, w, h1[u]);
            }
        };
        if (npair > 0) {
            for (int p = 0; p + 1 < npair; ++p) {              // block 2 p is in a
                issue(ray, b0, b1, (2 * p + 1) * RU);
                pin();
                consume(a0, a1, 2 * p * RU);
                pin();
                issue(ray, a0, a1, (2 * p + 2) * RU);
                pin();
                consume(b0, b1, (2 * p + 1) * RU);
                pin();
            }
            issue(ray, b0, b1, (2 * npair - 1) * RU);
            pin();
            consume(a0, a1, (2 * npair - 2) * RU);
            pin();
            if (pre) issue(nxt, a0, a1, 0);                    // the next group's first rows, behind this group's last
            pin();
            consume(b0, b1, (2 * npair - 1) * RU);
            pin();
        }
        for (int row = npair * 2 * RU; row < T; ++row) {
            const half8 h0 = __builtin_nontemporal_load(reinterpret_cast<const half8*>(ray.hp + (size_t)row * HC + off0));
            const half8 h1 = __builtin_nontemporal_load(reinterpret_cast<const half8*>(ray.hp + (size_t)row * HC + off1));
            const float w = wt[row];
            if (row < T - T % HID_BLOCK_ROWS) {                // (hid_sum.h: the rounding goes by the row, not by how it is loaded)
                hid_row_acc<true>(acc0, w, h0);
                hid_row_acc<true>(acc1, w, h1);
            } else {
                hid_row_acc<false>(acc0, w, h0);
                hid_row_acc<false>(acc1, w, h1);
            }
        }
        half8 o0, o1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o0[e] = (_Float16)acc0[e];
            o1[e] = (_Float16)acc1[e];
        }
        *reinterpret_cast<half8*>(hbar + ray.lray * HC + c0 * 8) = o0;
        if (live1) *reinterpret_cast<half8*>(hbar + ray.lray * HC + c1 * 8) = o1;
    }
}

template <int MODE>
int launch(const UnitArgs& args, const UnitGeo& geo, const __half* hid, __half* hbar, float* at_wt, float* logits, hipStream_t stream) {
    const int T = geo.V * geo.S;
    const size_t lds = unit_lds_bytes<MODE>() + (size_t)3 * TG * T * sizeof(float);
    CPN_REQUIRE(lds <= (size_t)LDS_MAX, CPN_E_SHAPE,
                "cpn_attend_units: V*S = %d needs %zu B of LDS (weights + 3 x 4 rays of logits / weights), the CU has %d", T, lds, LDS_MAX);
    auto kern = attend_units_kernel<MODE>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        if (e != hipSuccess) {
            cpn_set_error("cpn_attend_units: cannot reserve %d B of LDS: %s", LDS_MAX, hipGetErrorString(e));
            return (int)e;
        }
        attr_set = true;
    }
    const long long ngroups = geo.nunits / (geo.V * geo.nsblk);
    const int num_cu = cpn_stream_cus((void*)stream);          // persistent: one workgroup per CU, its ray groups its own
    const unsigned grid = (unsigned)std::min<long long>(ngroups, num_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(AU_THREADS), lds, stream, args, geo, hid, hbar, at_wt, logits);
    CPN_LAUNCH_CHECK("cpn_attend_units");
    return 0;
}

}  // namespace

extern "C" int cpn_attend_units(int mode, const float* loc8, const float* coords9, const float* w1, int ldw1, const float* b1,
                                const float* add, const uint16_t* w2, int ldw2, const float* b2, const uint16_t* wk2, int ldwk2,
                                const float* bk2, const float* w1b, int ldw1b, const float* b1b, const uint16_t* kh_u,
                                const uint16_t* hid, int B, int V, int R, int S, int ray0, int nrays, const float* lv_u,
                                uint16_t* hbar, float* at_wt, float* logits, void* stream) {
    CPN_REQUIRE(mode == 0 || mode == 2, CPN_E_ARG, "cpn_attend_units: mode must be 0 or 2 (got %d)", mode);
    CPN_REQUIRE(loc8 && coords9 && w1 && b1 && w2 && b2 && wk2 && bk2 && hid && hbar, CPN_E_ARG, "cpn_attend_units: null pointer");
    CPN_REQUIRE(mode == 0 ? kh_u != nullptr : (add && w1b && b1b), CPN_E_ARG, "cpn_attend_units: null pointer for mode %d", mode);
    CPN_REQUIRE(B > 0 && V == 2 && R > 0 && S > 0 && ldw1 >= 16 && ldw2 >= 128 && (ldw2 % 8) == 0 && ldwk2 >= 128 &&
                    (ldwk2 % 8) == 0 && (mode != 2 || ldw1b >= 16), CPN_E_SHAPE, "cpn_attend_units: bad shape");
    CPN_REQUIRE(ray0 >= 0 && nrays > 0 && (long long)ray0 + nrays <= (long long)B * R, CPN_E_ARG,
                "cpn_attend_units: ray range outside B*R");
    CPN_REQUIRE(((uintptr_t)kh_u % 16) == 0 && ((uintptr_t)w2 % 16) == 0 && ((uintptr_t)wk2 % 16) == 0 && ((uintptr_t)w1 % 16) == 0 &&
                    ((uintptr_t)w1b % 16) == 0 && ((uintptr_t)lv_u % 16) == 0 && ((uintptr_t)hid % 16) == 0 && ((uintptr_t)hbar % 16) == 0,
                CPN_E_ARG, "cpn_attend_units: fp16 operands, first-layer weights, hid and hbar must be 16-byte aligned");
    const UnitGeo geo = unit_geo(V, R, S, ray0, nrays);
    CPN_REQUIRE(geo.nunits * 16 < (1LL << 31), CPN_E_SHAPE, "cpn_attend_units: chunk too large for 32-bit indexing");
    const f32x4* lv_chunk = lv_u ? reinterpret_cast<const f32x4*>(lv_u) + (size_t)geo.group0 * V * geo.nsblk * 64 : nullptr;
    const UnitArgs args{loc8, coords9, w1, ldw1, b1, add, (const __half*)w2, ldw2, b2, (const __half*)wk2, ldwk2, bk2, w1b, ldw1b, b1b,
                        (const __half*)kh_u, nullptr, lv_chunk};
    return mode == 0 ? launch<0>(args, geo, (const __half*)hid, (__half*)hbar, at_wt, logits, (hipStream_t)stream)
                     : launch<2>(args, geo, (const __half*)hid, (__half*)hbar, at_wt, logits, (hipStream_t)stream);
}
