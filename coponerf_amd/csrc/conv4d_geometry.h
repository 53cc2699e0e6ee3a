// Geometry of one Conv4d layer (models/conv4d.py): the input volume, the filter, and the output sizes of its two separable
// branches, in ONE place for the forward (ufc_conv4d.hip) and the strided backward (ufc_strided_bwd.hip).
#pragma once
#include "common.h"

namespace {

struct SGeo {
    int B, Cin, Cout, Hq, Wq, Hs, Ws, k, s, p, Oq, Pq, Os, Ps;
    __host__ __device__ long long n_ps() const { return (long long)B * Cin * Hq * Wq * Os * Ps; }
    __host__ __device__ long long n_pq() const { return (long long)B * Cin * Oq * Pq * Hs * Ws; }
    __host__ __device__ long long npos() const { return (long long)Oq * Pq * Os * Ps; }
};

// size of a dim of n after the max-pool by s (ceil mode)
inline int pooled_size(int n, int s) { return (n + s - 1) / s; }

// Output sizes co(n) = (n + 2p - k) / s + 1 of the convolved pair of dims; false when they differ from the pooled sizes of
// the other pair: the two branches must meet on one output grid.
inline bool make_geo(int B, int Cin, int Cout, int Hq, int Wq, int Hs, int Ws, int k, int s, int p, SGeo* g) {
    auto co = [&](int n) { return (n + 2 * p - k) / s + 1; };
    *g = SGeo{B, Cin, Cout, Hq, Wq, Hs, Ws, k, s, p, co(Hq), co(Wq), co(Hs), co(Ws)};
    return g->Oq == pooled_size(Hq, s) && g->Pq == pooled_size(Wq, s) && g->Os == pooled_size(Hs, s) && g->Ps == pooled_size(Ws, s);
}

}  // namespace
