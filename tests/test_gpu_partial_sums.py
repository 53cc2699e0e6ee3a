"""The fixed-order reductions of csrc/partial_sum.h, held to their documented order.

Every user leaves its partial results in caller-owned scratch that survives the call.  Each test calls the entry, reads the
partials back in the layout stated beside the entry's `*_scratch` function, replays the documented order on the host in
float32 (numpy: one rounding per add; float64 for sum_partials_f64, the finish of the image-side units) and requires the
entry's result to be the same bits.  This holds even where the producing kernel is not bit-reproducible, because the sums
are taken over the partials that very run produced."""
import ctypes

import numpy as np
import pytest
import torch

from coponerf_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def replay_16x64(parts):
    """sum_partials_16x64 for parts (n_part, n_out): wave p adds partials p, p + 16, ... in ascending order from 0, then
    the 16 wave sums are added in the order 0 .. 15 from 0."""
    parts = np.ascontiguousarray(parts, dtype=np.float32)
    sh = np.zeros((16, parts.shape[1]), np.float32)
    for p in range(16):
        for b in range(p, parts.shape[0], 16):
            sh[p] += parts[b]
    v = np.zeros(parts.shape[1], np.float32)
    for q in range(16):
        v += sh[q]
    return v


def replay_slabs(parts):
    """sum_slabs_f32x4 for parts (nslab, ...): slab 0, then + slab 1, + slab 2, ..."""
    parts = np.ascontiguousarray(parts, dtype=np.float32)
    s = parts[0].copy()
    for q in range(1, parts.shape[0]):
        s += parts[q]
    return s


def replay_f64(parts, nt=64):
    """sum_partials_f64 for parts (n, ...) and a workgroup of nt threads: thread t adds partials t, t + nt, ... in ascending
    order from 0.0 in float64, then the xor butterfly 32, 16, .. 1 adds the 64 lanes of each wave.  Returns the nt / 64 wave
    sums, (nt / 64, ...)."""
    parts = np.ascontiguousarray(parts, dtype=np.float32).astype(np.float64)
    lanes = np.zeros((nt,) + parts.shape[1:], np.float64)
    for i in range(parts.shape[0]):
        lanes[i % nt] += parts[i]
    v = lanes.reshape((nt // 64, 64) + parts.shape[1:])
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ o]
    assert all(np.array_equal(v[:, 0], v[:, l], equal_nan=True) for l in range(64))     # every lane holds the sum
    return v[:, 0]


def _same_bits(got, want):
    return torch.equal(got.cpu().reshape(-1), torch.from_numpy(np.asarray(want, np.float32).reshape(-1)))


# partial counts: below 16 (empty waves), exactly 128 (one unrolled pass, no tail), above 128 with a remainder (22) that is
# not a multiple of 16
@pytest.mark.parametrize("B,G", [(1, 7), (2, 64), (2, 75)])
def test_conv_wgrad_planes_reducer_order(dev, B, G):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    Cin = Cout = 8
    H = W = 4
    x = syn.normal((B, Cin, G, H, W), seed=11).to(dev)
    dy = syn.normal((B, Cout, G, H, W), seed=12).to(dev)
    part = torch.zeros(_hip.lib().cpn_conv_wgrad_scratch(Cin, Cout), device=dev)
    dw, db = torch.empty(Cout, Cin, 3, 3, device=dev), torch.empty(Cout, device=dev)
    call("cpn_conv_wgrad_planes", x.data_ptr(), dy.data_ptr(), B, Cin, Cout, G, H, W, part.data_ptr(), dw.data_ptr(),
         db.data_ptr(), _st())
    nw, nblocks = Cout * Cin * 9, min(B * G, 512)
    assert nw + Cout == 584                                              # ten workgroups of 64 outputs, the last partly filled
    parts = part.cpu().numpy()[:nblocks * (nw + Cout)].reshape(nblocks, nw + Cout)
    want = replay_16x64(parts)
    assert float(np.abs(want).max()) > 0.0
    assert _same_bits(dw, want[:nw]) and _same_bits(db, want[nw:])


@pytest.mark.parametrize("B,H", [(1, 7), (2, 64), (2, 75)])
def test_dwconv_tokens_wgrad_reducer_order(dev, B, H):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    W, C = 4, 12
    x = syn.normal((B, H * W, C), seed=13).to(dev)
    dy = syn.normal((B, H * W, C), seed=14).to(dev)
    part = torch.zeros(_hip.lib().cpn_dwconv3x3_tokens_wgrad_scratch(B, H, C), device=dev)
    dw, db = torch.empty(C, 9, device=dev), torch.empty(C, device=dev)
    call("cpn_dwconv3x3_tokens_wgrad", x.data_ptr(), dy.data_ptr(), B, H, W, C, part.data_ptr(), dw.data_ptr(), db.data_ptr(),
         _st())
    want = replay_16x64(part.cpu().numpy().reshape(B * H, C * 10)).reshape(C, 10)        # 120 outputs (c, term)
    assert float(np.abs(want).max()) > 0.0
    assert _same_bits(dw, want[:, :9]) and _same_bits(db, want[:, 9])


# the two smallest cases of test_strided_conv4d_vjp_equals_library_graph (1 and 2 chunks: the chunk count is set inside
# the library, 4096 positions of B * npos each), and one that passes 128 chunks with a remainder of 8: 136 chunks
@pytest.mark.parametrize("B,n,k,s,p,cin", [(2, 10, 5, 4, 2, 2), (2, 13, 3, 2, 1, 1), (11, 30, 3, 2, 1, 1)])
def test_strided_conv4d_wgrad_reducer_order(dev, B, n, k, s, p, cin):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    cout, kk = 8, k * k
    o = (n + 2 * p - k) // s + 1
    assert o == -(-n // s)
    x = torch.randn(B, cin, n, n, n, n, generator=torch.Generator().manual_seed(5)).to(dev)
    dy = torch.randn(B, cout, o, o, o, o, generator=torch.Generator().manual_seed(6)).to(dev)
    wq = syn.normal((cout, cin, k, k), seed=15).to(dev)
    ws = syn.normal((cout, cin, k, k), seed=16).to(dev)
    scratch = torch.zeros(_hip.lib().cpn_conv4d_strided_bwd_scratch(B, cin, cout, n, n, n, n, k, s, p), device=dev)
    gwq, gws, gb = torch.empty_like(wq), torch.empty_like(ws), torch.empty(cout, device=dev)
    call("cpn_conv4d_strided_bwd", x.data_ptr(), dy.data_ptr(), wq.data_ptr(), ws.data_ptr(), B, cin, cout, n, n, n, n, k, s,
         p, scratch.data_ptr(), 0, gwq.data_ptr(), gws.data_ptr(), gb.data_ptr(), _st())
    nvol = 2 * B * cin * n * n * o * o                                   # n_ps + n_pq
    nch = -(-(B * o ** 4) // 4096)
    print(f"strided Conv4d weight gradient: {nch} chunk partials at B={B} n={n} k={k} s={s}")
    na, ntap = cout * cin, 2 * kk
    off = 2 * nvol + (nvol + 3) // 4
    assert scratch.numel() == off + nch * (ntap * na + cout)
    sc = scratch.cpu().numpy()
    part = sc[off:off + nch * ntap * na].reshape(nch, ntap * na)
    partb = sc[off + nch * ntap * na:].reshape(nch, cout)
    want = replay_16x64(np.concatenate([part, partb], axis=1))
    assert float(np.abs(want).max()) > 0.0
    w = want[:ntap * na].reshape(2, kk, na)                               # [branch][i*k + j][o * Cin + c]
    assert _same_bits(gwq, w[0].T) and _same_bits(gws, w[1].T) and _same_bits(gb, want[ntap * na:])


# R = 300: one slab; R = 1100: four (the slab count is capped by R / 256)
@pytest.mark.parametrize("R", [300, 1100])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_wgrad_slab_order(dev, R, bias):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    O, I = 68, 72
    dY = syn.normal((R, O), seed=17).to(dev)
    X = syn.normal((R, I), seed=18).to(dev)
    floats = _hip.lib().cpn_wgrad_f32_scratch_floats(R, O, I)
    assert floats % (O * I + O) == 0
    nslab = floats // (O * I + O)
    assert nslab == (1 if R == 300 else 4)
    scratch = torch.zeros(floats, device=dev)
    dW, db = torch.empty(O, I, device=dev), torch.empty(O, device=dev)
    call("cpn_wgrad_f32", dY.data_ptr(), O, X.data_ptr(), I, R, O, I, dW.data_ptr(), db.data_ptr() if bias else 0,
         scratch.data_ptr(), _st())
    sc = scratch.cpu().numpy()
    want = replay_slabs(sc[:nslab * O * I].reshape(nslab, O * I))
    assert float(np.abs(want).max()) > 0.0
    assert _same_bits(dW, want)
    if bias:
        assert _same_bits(db, replay_slabs(sc[nslab * O * I:].reshape(nslab, O)))


@pytest.mark.parametrize("scale", [3.0, None])
def test_tall_wgrad_slab_order(dev, scale):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    M, N, K = 1000, 208, 128
    g = torch.Generator().manual_seed(7)
    dY = (torch.randn(M, N, generator=g) * 0.5).half().to(dev)
    X = torch.randn(M, K, generator=g).half().to(dev)
    floats = _hip.lib().cpn_wgrad_tall_scratch(N, K)
    nslab = floats // (N * K)
    assert nslab > 1 and floats == nslab * N * K
    part = torch.zeros(floats, device=dev)
    dW = torch.empty(N, K, device=dev)
    sc = torch.tensor([scale], device=dev) if scale is not None else None
    call("cpn_wgrad_tall_f16", dY.data_ptr(), N, X.data_ptr(), K, M, N, K, sc.data_ptr() if sc is not None else 0,
         part.data_ptr(), dW.data_ptr(), _st())
    want = replay_slabs(part.cpu().numpy().reshape(nslab, N * K))
    assert float(np.abs(want).max()) > 0.0
    if scale is not None:
        want = want * (np.float32(1.0) / np.float32(scale))              # the kernel's own two roundings: 1 / scale, then the product
    assert want.dtype == np.float32
    assert _same_bits(dW, want)


# ---------------------------------------------------------------------- sum_partials_f64: the image-side units' finishes
# 9 tiles of 16 x 32: one trip of the strided loop for nine lanes, none for the rest; 72 tiles: a second trip for lanes 0 .. 7
@pytest.mark.parametrize("N,H,W", [(2, 41, 75), (1, 144, 256)])
def test_image_metrics_finish_order(dev, N, H, W):
    """The mse and ssim columns (psnr goes through the device's log: tests/test_gpu_metrics.py holds it)."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    from tests import metrics_ref as mr
    pred, target = (torch.from_numpy(a).to(dev) for a in mr.make_case("textured", N, H, W))
    ntile = -(-H // 16) * -(-W // 32)
    part = torch.zeros(_hip.lib().cpn_image_metrics_scratch(N, H, W), device=dev)
    assert part.numel() == N * ntile * 2 and ntile == (9 if H == 41 else 72)
    out = torch.empty(N, 3, device=dev)
    call("cpn_image_metrics", pred.data_ptr(), target.data_ptr(), N, H, W, part.data_ptr(), out.data_ptr(), _st())
    s = replay_f64(part.cpu().numpy().reshape(N, ntile, 2).transpose(1, 0, 2))[0]        # (N, [squared error, sum of S])
    assert float(np.abs(s).min()) > 0.0
    assert _same_bits(out[:, 0], s[:, 0] / (3.0 * H * W))
    assert _same_bits(out[:, 2], s[:, 1] / (3.0 * (H - 10) * (W - 10)))


def test_ssim_warp_finish_order(dev):
    """The per-item `sums` (loss and 1 / (3 den) add fp32 divisions: tests/test_gpu_ssim_warp.py holds them).  72 blocks."""
    from coponerf_amd import _hip, losses
    from coponerf_amd._hip import call
    from tests import ssim_ref as R
    B, H, W, s = 1, 144, 256, 4
    rgb, f0, f1 = (t.to(dev) for t in R.case(B, H, W, s))
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = (((ys + xs) % 3) != 0)[None, None].expand(B, 2, H, W).contiguous().to(dev)
    win = losses.gaussian_window().to(dev)
    nblk = _hip.lib().cpn_ssim_warp_blocks(H, W)
    assert nblk == 72
    coords, maps = torch.empty(2 * B, 2, H, W, device=dev), torch.empty(2 * B, 9, H, W, device=dev)
    part = torch.zeros(2 * B, nblk, 2, device=dev)
    sums, loss, inv = torch.empty(2 * B, 2, device=dev), torch.empty(2, device=dev), torch.empty(2, device=dev)
    call("cpn_ssim_warp", rgb.data_ptr(), f0.data_ptr(), f1.data_ptr(), mask.data_ptr(), win.data_ptr(), B, H, W, H // s, W // s,
         coords.data_ptr(), maps.data_ptr(), part.data_ptr(), sums.data_ptr(), loss.data_ptr(), inv.data_ptr(), _st())
    want = replay_f64(part.cpu().numpy().transpose(1, 0, 2))[0]                           # (item, [num, den])
    assert float(np.abs(want).min()) > 0.0
    assert _same_bits(sums, want)


def test_lpips_head_finish_order(dev):
    """C = 64, N = 2, a 65 x 64 map (65 workgroups per image: a second trip for lane 0) and a 5 x 7 map (one) in one call:
    per_layer is each layer's sum over its pixel count, out their sum in layer order."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    from tests import lpips_ref as lr
    N, C, shapes = 2, 64, ((65, 64), (5, 7))
    maps, lins = zip(*[lr.make_maps(N, C, h, w, seed=40 + k) for k, (h, w) in enumerate(shapes)])
    maps, lins = [m.to(dev) for m in maps], [l.to(dev) for l in lins]
    ints, ptrs = ctypes.c_int * 2, ctypes.c_void_p * 2
    hs, ws, cs = ints(*[h for h, _ in shapes]), ints(*[w for _, w in shapes]), ints(C, C)
    nblk = [-(-(h * w) // 64) for h, w in shapes]
    n = _hip.lib().cpn_lpips_head_scratch(N, 2, hs, ws)
    assert nblk == [65, 1] and n == N * sum(nblk)
    part, out, per = torch.zeros(n, device=dev), torch.empty(N, device=dev), torch.empty(N, 5, device=dev)
    call("cpn_lpips_head", ptrs(*[m.data_ptr() for m in maps]), ptrs(*[l.data_ptr() for l in lins]), cs, hs, ws, 2, N,
         part.data_ptr(), out.data_ptr(), per.data_ptr(), _st())
    p, off = part.cpu().numpy(), 0
    want, total = np.zeros((N, 5)), np.zeros(N)
    for k, (h, w) in enumerate(shapes):                                                   # layer k: N x nblk[k] floats
        want[:, k] = replay_f64(p[off:off + N * nblk[k]].reshape(N, nblk[k]).T)[0] / float(h * w)
        total = total + want[:, k]
        off += N * nblk[k]
    assert float(want[:, :2].min()) > 0.0
    assert _same_bits(per, want) and _same_bits(out, total)


# one workgroup; 257: thread 0 of the finish's 256 makes a second trip.  Then the four wave sums as (0 + 1) + (2 + 3).
@pytest.mark.parametrize("rows,S", [(5, 37), (8200, 8)])
def test_attention_entropy_finish_order(dev, rows, S):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    w = torch.softmax(torch.randn(rows, S, generator=torch.Generator().manual_seed(9)), dim=-1).to(dev)
    nblk = _hip.lib().cpn_attention_entropy_blocks(rows)
    assert nblk == (1 if rows == 5 else 257)
    part, out = torch.zeros(nblk, device=dev), torch.empty(1, device=dev)
    call("cpn_attention_entropy", w.data_ptr(), rows, S, 0, part.data_ptr(), out.data_ptr(), _st())
    v = replay_f64(part.cpu().numpy(), nt=256)
    want = ((v[0] + v[1]) + (v[2] + v[3])) / float(rows)
    assert want > 0.0
    assert _same_bits(out, want)
