"""cmx_gemm (csrc/gemm.hip) against a plain PyTorch fp32 reference of the same op.

Covers the three GEMMs of a layer (forward NT, dgrad with a transposed B, wgrad with both
operands transposed), ragged M / N / K (K = 152 is the padded 7x7x3 patch-embed K,
N = 40 the NYUv2 classifier), every epilogue (bias, GELU / ReLU, DropPath-scaled residual,
fp32 store / accumulate) and both storage dtypes.  Tolerances: fp32 mode 1e-5 relative
(exact fp32 MFMA, summation order differs); bf16 mode 1e-2 relative (bf16 output
rounding, fp32 accumulation)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30)).item()


def ref_epi(acc, bias, act, residual, rscale, rps):
    v = acc + (bias[:, None, :] if bias is not None else 0)
    v = {"none": v, "gelu": F.gelu(v), "relu": F.relu(v)}[act]
    if residual is not None:
        G, M = v.shape[:2]
        s = torch.ones(G * M, device=v.device) if rscale is None else rscale.repeat_interleave(rps)
        v = residual.float() + s.view(G, M, 1) * v
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("G,M,N,K", [(2, 300, 64, 64), (2, 1000, 128, 152), (1, 777, 40, 512), (2, 256, 320, 1280),
                                     (1, 130, 520, 24), (4, 512, 512, 300), (2, 64, 64, 1203)])
@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_gemm_layouts(dev, dtype, G, M, N, K, tA, tB):
    """K = 300 / 1203 with both operands transposed: the bf16 fast path takes any K there (k is
    the row index); the groups are packed back to back, so a k-row past K would read the next
    group's rows (the FFM k^T v / u^T dout products over 300-token images)."""
    torch.manual_seed(0)
    if (tA and M % 8) or (tB and N % 8):
        pytest.skip("transposed operand needs its contiguous dim % 8 == 0")
    A = torch.randn(G, M, K, device="cuda").to(dtype)
    B = torch.randn(G, N, K, device="cuda").to(dtype)
    Av = A.transpose(1, 2).contiguous().transpose(1, 2) if tA else A
    Bv = B.transpose(1, 2).contiguous().transpose(1, 2) if tB else B
    from rgbx_semantic_segmentation_amd import kernels as Kn
    C = torch.empty(G, M, N, device="cuda", dtype=dtype)
    Kn.gemm(Av, Bv, C)
    ref = torch.bmm(A.float(), B.float().transpose(1, 2))
    assert rel(C, ref) < (1e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["none", "gelu", "relu"])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("K", [96, 2048])
def test_gemm_epilogues(dev, dtype, act, res, K):
    """K = 2048 on a 600 x 192 output is an under-filled 64 x 64 problem with a short k-loop: it runs
    as KW = 2 k-group blocks (GEMM_SPLITKW), no split-K and no reducer, and the epilogue runs in the
    tile kernel.  The reducer's epilogue is covered by tests/test_gpu_gemm_exact.py (red_* cases)."""
    torch.manual_seed(1)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    G, M, N, rps = 2, 600, 192, 300
    A = torch.randn(G, M, K, device="cuda").to(dtype)
    B = torch.randn(G, N, K, device="cuda").to(dtype) * (1.0 / K ** 0.5)
    bias = torch.randn(G, N, device="cuda")
    R = torch.randn(G, M, N, device="cuda").to(dtype) if res else None
    s = torch.tensor([0.0, 1.25, 1.25, 0.0], device="cuda") if res else None
    C = torch.empty(G, M, N, device="cuda", dtype=dtype)
    Kn.gemm(A, B, C, bias=bias, residual=R, rscale=s, rows_per_sample=rps, act=act)
    ref = ref_epi(torch.bmm(A.float(), B.float().transpose(1, 2)), bias, act, R, s, rps)
    assert rel(C, ref) < (1e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K,res", [(96, True), (2048, True), (128, False)])
def test_gemm_relu_mask_epilogue(dev, dtype, K, res):
    """ReLU-backward mask epilogue (CrossPath's channel_proj ReLU, net_utils.py:273-274):
    C = (R + A B^T) * [mask > 0], in place over a column half of a wider buffer (the FFM's
    [dy | du] gradient), through the tile path; K = 2048 runs as KW = 2 k-group blocks (no split-K,
    no reducer: the reducer's mask epilogue is covered by tests/test_gpu_gemm_exact.py)."""
    torch.manual_seed(9)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    G, M, N = 2, 600, 96
    A = torch.randn(G, M, K, device="cuda").to(dtype)
    B = (torch.randn(G, N, K, device="cuda") / K ** 0.5).to(dtype)
    buf = torch.randn(G, M, 2 * N, device="cuda").to(dtype)
    act = torch.relu(torch.randn(G, M, 2 * N, device="cuda")).to(dtype)
    C, mask = buf[..., N:], act[..., N:]
    R0 = C.float().clone()
    Kn.gemm(A, B, C, residual=C if res else None, mask=mask)
    ref = torch.bmm(A.float(), B.float().transpose(1, 2)) + (R0 if res else 0)
    ref = ref * (mask.float() > 0)
    assert rel(C, ref) < (1e-5 if dtype == torch.float32 else 1e-2)
    assert bool((C.float()[mask.float() <= 0] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gemm_fp32_out_and_accumulate(dev, dtype):
    torch.manual_seed(2)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    G, M, N, K = 2, 4800, 64, 256          # wgrad-shaped: dW (N x K) = dy^T x over M tokens
    dy = torch.randn(G, M, N, device="cuda").to(dtype)
    x = torch.randn(G, M, K, device="cuda").to(dtype)
    W = torch.empty(G, N, K, device="cuda")
    Kn.gemm(dy.transpose(1, 2), x.transpose(1, 2), W, out_mode=1)
    ref = torch.bmm(dy.float().transpose(1, 2), x.float())
    assert rel(W, ref) < 1e-5
    Kn.gemm(dy.transpose(1, 2), x.transpose(1, 2), W, out_mode=2)
    assert rel(W, 2 * ref) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gemm_two_segment_A(dev, dtype):
    """Linear on cat(x1, x2) without the cat (end_proj / ChannelEmbed)."""
    torch.manual_seed(3)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    G, M, N, K1, K2 = 2, 700, 160, 64, 96
    x1 = torch.randn(G, M, K1, device="cuda").to(dtype)
    x2 = torch.randn(G, M, K2, device="cuda").to(dtype)
    W = torch.randn(G, N, K1 + K2, device="cuda").to(dtype)
    b = torch.randn(G, N, device="cuda")
    C = torch.empty(G, M, N, device="cuda", dtype=dtype)
    Kn.gemm(x1, W, C, bias=b, A2=x2)
    ref = torch.bmm(torch.cat([x1, x2], -1).float(), W.float().transpose(1, 2)) + b[:, None, :]
    assert rel(C, ref) < (1e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("splitk", [1, 7, 32])
@pytest.mark.parametrize("accumulate", [False, True])
def test_gemm_wgrad_splitk_bias_grad(dev, dtype, splitk, accumulate):
    """dW = dy^T x split over tokens, written into a column slice of a wider gradient
    buffer (K-split Linear), with the bias gradient from the virtual ones column."""
    torch.manual_seed(4)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    G, Mtok, N, Kx, Ktot, k0 = 2, 9600, 64, 128, 320, 64
    dy = torch.randn(G, Mtok, N, device="cuda").to(dtype)
    x = torch.randn(G, Mtok, Kx, device="cuda").to(dtype)
    Wg = torch.randn(G, N, Ktot, device="cuda")
    bg = torch.randn(G, N, device="cuda")
    W0, b0 = Wg.clone(), bg.clone()
    Kn.gemm(dy.transpose(1, 2), x.transpose(1, 2), Wg[:, :, k0:k0 + Kx], out_mode=2 if accumulate else 1,
            dbias=bg, splitk=splitk)
    refW = torch.bmm(dy.float().transpose(1, 2), x.float())
    refb = dy.float().sum(1)
    if accumulate:
        refW, refb = refW + W0[:, :, k0:k0 + Kx], refb + b0
    assert rel(Wg[:, :, k0:k0 + Kx], refW) < 1e-5
    assert rel(bg, refb) < 1e-5
    assert torch.equal(Wg[:, :, :k0], W0[:, :, :k0]) and torch.equal(Wg[:, :, k0 + Kx:], W0[:, :, k0 + Kx:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1)])
def test_gemm_unaligned_dims(dev, dtype, tA, tB):
    """Row strides / reduction lengths that are not whole 16-B chunks (K = 9 classes of the
    B0 classifier's dgrad, lda = 9) take the element-wise generic path."""
    torch.manual_seed(5)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    G, M, N, K = 1, 768, 512, 9
    A = torch.randn(G, M, K, device="cuda").to(dtype)
    B = torch.randn(G, N, K, device="cuda").to(dtype)
    Bv = B.transpose(1, 2).contiguous().transpose(1, 2) if tB else B
    C = torch.empty(G, M, N, device="cuda", dtype=dtype)
    Kn.gemm(A, Bv, C)
    ref = torch.bmm(A.float(), B.float().transpose(1, 2))
    assert rel(C, ref) < (1e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("G,M,N,K", [(2, 38400, 256, 64), (1, 38400, 512, 2048), (2, 600, 64, 4096),
                                     (2, 2400, 320, 1280), (2, 64, 256, 38400)])
@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 1)])
def test_gemm_step_shapes_bf16(dev, G, M, N, K, tA, tB):
    """The bf16 LDS-DMA path on the shapes of the B2 step (census in scripts/gemm_census.py):
    large-M forward / dgrad tiles, small-output split-K and token-reduction wgrads."""
    torch.manual_seed(6)
    from rgbx_semantic_segmentation_amd import kernels as Kn
    dt = torch.bfloat16
    A = torch.randn(G, M, K, device="cuda").to(dt)
    B = torch.randn(G, N, K, device="cuda").to(dt)
    Av = A.transpose(1, 2).contiguous().transpose(1, 2) if tA else A
    Bv = B.transpose(1, 2).contiguous().transpose(1, 2) if tB else B
    C = torch.empty(G, M, N, device="cuda", dtype=torch.float32)
    Kn.gemm(Av, Bv, C, out_mode=1)
    ref = torch.bmm(A.float(), B.float().transpose(1, 2))
    assert rel(C, ref) < 1e-5


@pytest.mark.parametrize("Cin,Cout,k,st,pad,H,W", [(64, 128, 3, 2, 1, 30, 40), (128, 320, 3, 2, 1, 15, 20),
                                                   (64, 64, 8, 8, 0, 120, 160), (320, 320, 2, 2, 0, 30, 40)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_implicit_conv(dev, Cin, Cout, k, st, pad, H, W, dt):
    """im2col-free conv (cmx_conv_implicit_fwd) and its per-tap grouped weight gradient
    (deferred.conv_wgrad) against torch fp32 conv2d: OverlapPatchEmbed k3 s2 p1 and the SRA
    spatial-reduction conv kR sR (dual_segformer.py:95-96, 196-197).  bf16 tolerance 1e-2."""
    from rgbx_semantic_segmentation_amd import deferred
    from rgbx_semantic_segmentation_amd import kernels as K
    torch.manual_seed(3)
    G, NIg = 2, 2
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    x = torch.randn(G * NIg, H, W, Cin, device=dev).to(dt)
    Wt = (torch.randn(G, Cout, k, k, Cin, device=dev) / math.sqrt(k * k * Cin)).to(dt)
    b = torch.randn(G, Cout, device=dev)
    y = torch.empty(G, NIg * Ho * Wo, Cout, device=dev, dtype=dt)
    M = NIg * Ho * Wo
    sk = K.query("cmx_gemm_splitk", G, M, Cout, k * k * Cin, 0, 1)
    ws = K._ws(K.query("cmx_gemm_workspace", G, M, Cout, sk), dev) if sk > 1 else None
    K.call("cmx_conv_implicit_fwd", K.ptr(x), K.ptr(Wt), K.ptr(y), K.ptr(b), K.ptr(ws), G, NIg, H, W, Cin, k, k, st,
           pad, Ho, Wo, Cout, NIg * H * W * Cin, Wt[0].numel(), y.stride(0), Cout, sk, K.dtype_code(x), K.stream())
    xr = x.float().view(G, NIg, H, W, Cin).permute(0, 1, 4, 2, 3)
    for g in range(G):
        ref = F.conv2d(xr[g], Wt[g].float().permute(0, 3, 1, 2), b[g], stride=st, padding=pad)   # (NIg, Cout, Ho, Wo)
        got = y[g].view(NIg, Ho, Wo, Cout).permute(0, 3, 1, 2)
        assert rel(got, ref) < 1e-2, rel(got, ref)
    # weight gradient of every tap in one grouped launch
    dy = torch.randn(G, NIg * Ho * Wo, Cout, device=dev).to(dt)
    Wg = torch.full((G, Cout, k * k * Cin), float("nan"), device=dev)
    bg = torch.full((G, Cout), float("nan"), device=dev)
    assert deferred.conv_wgrad(dy, x, Wg, bg, (G, NIg, H, W, Cin, k, k, st, pad, Ho, Wo))
    deferred.flush()
    torch.cuda.synchronize()
    for g in range(G):
        wr = Wt[g].float().permute(0, 3, 1, 2).clone().requires_grad_(True)
        xg = xr[g].clone()
        out = F.conv2d(xg, wr, None, stride=st, padding=pad)
        out.backward(dy[g].float().view(NIg, Ho, Wo, Cout).permute(0, 3, 1, 2))
        ref_w = wr.grad.permute(0, 2, 3, 1).reshape(Cout, -1)
        assert rel(Wg[g], ref_w) < 1e-2, rel(Wg[g], ref_w)
        assert rel(bg[g], dy[g].float().sum(0)) < 1e-2


@pytest.mark.parametrize("case", ["qkv1", "qkv3", "qkv4", "decoder", "mixed"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_gemm_multi_matches_single(dev, case, dt):
    """Independent GEMMs as ONE launch (cmx_gemm_plan + cmx_gemm_multi; functions._gemm_group):
    Attention.q beside .kv at the B2 stage-1 / 3 / 4 shapes (forward with bias, and the dgrads),
    the decoder's four linear_c products, and a mix with a problem that is not eligible (split-K)
    and runs on its own.  Each output against torch fp32 on the same operands (1e-2 relative,
    16-bit output rounding)."""
    from rgbx_semantic_segmentation_amd import functions as Fn
    torch.manual_seed(11)
    shapes = {"qkv1": [(2, 38400, 64, 64), (2, 600, 128, 64)],
              "qkv3": [(2, 2400, 320, 320), (2, 600, 640, 320)],
              "qkv4": [(2, 600, 512, 512), (2, 600, 1024, 512)],
              "decoder": [(1, 38400, 512, 64), (1, 9600, 512, 128), (1, 2400, 512, 320), (1, 600, 512, 512)],
              "mixed": [(2, 2400, 320, 320), (1, 64, 64, 8192), (2, 600, 128, 64)]}[case]
    for dgrad in (False, True):
        jobs, refs = [], []
        for G, M, N, Kd in shapes:
            A = torch.randn(G, M, Kd, device=dev).to(dt)
            W = (torch.randn(G, N, Kd, device=dev) / math.sqrt(Kd)).to(dt)
            if dgrad:                      # dx (G, M, Kd) = dy (G, M, N) @ W (G, N, Kd)
                dy = torch.randn(G, M, N, device=dev).to(dt)
                C = torch.empty(G, M, Kd, device=dev, dtype=dt)
                jobs.append(dict(A=dy, B=W.transpose(1, 2), C=C))
                refs.append((C, torch.bmm(dy.float(), W.float())))
            else:
                b = torch.randn(G, N, device=dev)
                C = torch.empty(G, M, N, device=dev, dtype=dt)
                jobs.append(dict(A=A, B=W, C=C, bias=b))
                refs.append((C, torch.bmm(A.float(), W.float().transpose(1, 2)) + b[:, None, :]))
        Fn._gemm_group(jobs)
        torch.cuda.synchronize()
        for C, ref in refs:
            assert rel(C, ref) < 1e-2, (case, dgrad, C.shape, rel(C, ref))


@pytest.mark.parametrize("G,B,H,W,N", [(2, 2, 480, 640, 64), (2, 1, 64, 96, 32), (1, 3, 37, 203, 64),
                                       (2, 2, 4, 4, 64), (2, 1, 100, 260, 48)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_pe1_direct_conv(dev, G, B, H, W, N, dt):
    """Stage-1 patch embed straight from the fp32 NCHW batches (patch_embed1.hip: Conv2d 3 -> N,
    k7 s4 p3, dual_segformer.py:196-197) against torch conv2d on the 16-bit-rounded image and
    weights (fp64 reference: the kernel rounds the patch values to the storage type, accumulates
    in fp32): output 1e-2 relative (16-bit output rounding); weight / bias gradient from the
    per-workgroup slabs + grouped reduce 1e-4 relative (fp32 sums of exact 16-bit products).
    Ragged row tiles (Wo % 64 != 0), a 1 x 1 output grid, G = 1, N = 32 / 48 (B0 / padded); for
    N = 32 / 64 the LayerNorm epilogue (OverlapPatchEmbed.norm) against cmx_layernorm_fwd on the
    same stored conv output, bit for bit."""
    from rgbx_semantic_segmentation_amd import deferred
    from rgbx_semantic_segmentation_amd import kernels as K
    torch.manual_seed(5)
    Kp = 152
    Ho, Wo = (H + 6 - 7) // 4 + 1, (W + 6 - 7) // 4 + 1
    img = [torch.randn(B, 3, H, W, device=dev) for _ in range(G)]
    Wt = torch.zeros(G, N, Kp, device=dev, dtype=dt)
    Wt[:, :, :147] = (torch.randn(G, N, 147, device=dev) / math.sqrt(147)).to(dt)
    bias = torch.randn(G, N, device=dev)
    y = torch.full((G, B * Ho * Wo, N), float("nan"), device=dev, dtype=dt)
    fuse_ln = N in (32, 64)
    gamma = torch.randn(G, N, device=dev) if fuse_ln else None
    beta = torch.randn(G, N, device=dev) if fuse_ln else None
    y_ln = torch.empty_like(y) if fuse_ln else None
    mean = torch.empty(G * B * Ho * Wo, device=dev) if fuse_ln else None
    rstd = torch.empty_like(mean) if fuse_ln else None
    K.call("cmx_pe1_conv_fwd", K.ptr(img[0]), K.ptr(img[-1]) if G == 2 else 0, K.ptr(Wt), K.ptr(bias), K.ptr(y), G, B,
           3, H, W, 7, 7, 4, 3, Ho, Wo, N, Kp, Wt.stride(0), bias.stride(0), y.stride(0), K.ptr(gamma), K.ptr(beta),
           K.ptr(y_ln), K.ptr(mean), K.ptr(rstd), N, 1e-5, K.dtype_code(y), K.stream())
    if fuse_ln:
        # the fused LayerNorm epilogue (OverlapPatchEmbed.norm) = cmx_layernorm_fwd on the stored y, bit for bit
        ref_ln, ref_mean, ref_rstd = K.layernorm_fwd(y, gamma, beta, 1e-5, G=G)
        torch.cuda.synchronize()
        assert torch.equal(y_ln, ref_ln.view_as(y_ln)), (y_ln.float() - ref_ln.view_as(y_ln).float()).abs().max()
        assert torch.equal(mean, ref_mean.view(-1)) and torch.equal(rstd, ref_rstd.view(-1))
    dy = torch.randn(G, B * Ho * Wo, N, device=dev).to(dt)
    nblk = K.query("cmx_pe1_conv_wgrad_nblk", B, Ho, Wo)
    ws = torch.empty(G, nblk, N, Kp + 1, device=dev)
    K.call("cmx_pe1_conv_wgrad", K.ptr(dy), K.ptr(img[0]), K.ptr(img[-1]) if G == 2 else 0, K.ptr(ws), G, B, 3, H, W,
           7, 7, 4, 3, Ho, Wo, N, Kp, dy.stride(0), K.dtype_code(dy), K.stream())
    Wg = torch.full((G, N, Kp), float("nan"), device=dev)
    bg = torch.full((G, N), float("nan"), device=dev)
    deferred.reduce(ws, Wg, bg, G, nblk, nblk * N * (Kp + 1), N * (Kp + 1), N, Kp + 1, Kp, Wg.stride(0), Wg.stride(1),
                    bg.stride(0), 1)
    deferred.flush()
    torch.cuda.synchronize()
    for g in range(G):
        xr = img[g].to(dt).double()
        wr = Wt[g, :, :147].double().view(N, 3, 7, 7).requires_grad_(True)
        ref = F.conv2d(xr, wr, bias[g].double(), stride=4, padding=3)
        got = y[g].view(B, Ho, Wo, N).permute(0, 3, 1, 2)
        assert rel(got, ref) < 1e-2, rel(got, ref)
        ref.backward(dy[g].double().view(B, Ho, Wo, N).permute(0, 3, 1, 2))
        assert rel(Wg[g, :, :147], wr.grad.reshape(N, 147)) < 1e-4, rel(Wg[g, :, :147], wr.grad.reshape(N, 147))
        assert Wg[g, :, 147:].abs().max().item() == 0.0          # the padding columns' gradient
        assert rel(bg[g], dy[g].double().sum(0)) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("GB,heads,N,D", [(4, 2, 4800, 64), (4, 5, 1200, 64), (2, 8, 300, 64), (4, 1, 333, 32)])
def test_gemm_h2_per_head(dev, dtype, GB, heads, N, D):
    """cmx_gemm_h2 (two-level batch) on the FFM cross attention's per-head views: the heads are
    column slices of token rows (net_utils.py:206-212).  k_h^T v_h (fp32 out, split-K over tokens)
    and u_h @ ctx_h into a strided output slice, against torch on the same views."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    from rgbx_semantic_segmentation_amd.functions import _heads
    torch.manual_seed(7)
    C = heads * D
    kv = torch.randn(2, GB // 2 * N, 2 * C, device=dev).to(dtype)
    kh, vh = _heads(kv, GB, N, heads, D), _heads(kv, GB, N, heads, D, C)
    KV = torch.empty(GB, heads, D, D, device=dev)
    Kn.gemm_h2(kh.transpose(2, 3), vh.transpose(2, 3), KV, out_mode=1)
    ref = kh.float().transpose(2, 3) @ vh.float()
    assert rel(KV, ref) < (1e-5 if dtype == torch.float32 else 2e-3), rel(KV, ref)
    ctxT = torch.randn(GB, heads, D, D, device=dev).to(dtype)
    wide = torch.zeros(2, GB // 2 * N, 2 * C, device=dev, dtype=dtype)      # output: second half of wider rows
    out = _heads(wide[..., C:], GB, N, heads, D)
    Kn.gemm_h2(kh, ctxT, out)
    ref = kh.float() @ ctxT.float().transpose(2, 3)
    assert rel(out, ref) < (1e-5 if dtype == torch.float32 else 1e-2), rel(out, ref)
    assert not wide[..., :C].abs().any()                                     # the other half untouched


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("G,M,N,K,res", [(2, 38400, 64, 256, True), (2, 9600, 128, 512, True), (1, 130, 128, 64, True),
                                         (2, 4800, 32, 128, True), (2, 1000, 64, 64, True),
                                         (1, 77, 128, 128, False), (2, 2400, 128, 128, True),
                                         # stage-1 proj -> norm2 (1200 tiles, K = 64): the streaming grid
                                         (2, 38400, 64, 64, True)])
def test_gemm_ln_tail(dev, dtype, G, M, N, K, res):
    """cmx_gemm_ln: the GEMM output is the plain launch's, bit for bit, and the LayerNorm in its
    epilogue (N <= 128: one tile spans the row) sums exactly as ln_fwd_kernel -- statistics and y
    bit-identical to cmx_layernorm_fwd on that output.  Wider rows are refused (None)."""
    from rgbx_semantic_segmentation_amd import kernels as Kk
    torch.manual_seed(1)
    A = torch.randn(G, M, K, device="cuda").to(dtype)
    W = (torch.randn(G, N, K, device="cuda") / math.sqrt(K)).to(dtype)
    bias = torch.randn(G, N, device="cuda")
    R = torch.randn(G, M, N, device="cuda").to(dtype) if res else None
    rps = max(1, M // 2)
    rscale = (torch.rand(G * M // rps, device="cuda") + 0.5) if res else None
    gamma = torch.rand(G, N, device="cuda") + 0.5
    beta = torch.randn(G, N, device="cuda")
    for rep in range(3):
        C = torch.empty(G, M, N, device="cuda", dtype=dtype)
        out = Kk.gemm_ln(A, W, C, gamma, beta, 1e-6, bias=bias, residual=R, rscale=rscale, rows_per_sample=rps)
        assert out is not None, "gemm_ln refused an eligible problem"
        y, mean, rstd = out
        C0 = torch.empty_like(C)
        Kk.gemm(A, W, C0, bias=bias, residual=R, rscale=rscale, rows_per_sample=rps)
        torch.cuda.synchronize()
        assert torch.equal(C, C0), rep
        y0, m0, r0 = Kk.layernorm_fwd(C0, gamma, beta, 1e-6, G=G)
        torch.cuda.synchronize()
        assert (mean.flatten() - m0).abs().max().item() < 1e-5 * max(1.0, m0.abs().max().item())
        assert ((rstd.flatten() - r0).abs() / r0).max().item() < 1e-5
        assert torch.equal(mean.flatten(), m0) and torch.equal(rstd.flatten(), r0) and torch.equal(y, y0), rep
    Cw = torch.empty(G, M, 320, device="cuda", dtype=dtype)
    Ww = (torch.randn(G, 320, K, device="cuda") / math.sqrt(K)).to(dtype)
    assert Kk.gemm_ln(A, Ww, Cw, torch.ones(G, 320, device="cuda"), torch.zeros(G, 320, device="cuda"), 1e-6) is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("G,M,N,K,res,dy2", [(2, 38400, 64, 256, True, False), (2, 9600, 128, 512, True, True),
                                             (2, 4800, 32, 128, True, False), (1, 77, 128, 512, False, True),
                                             (2, 1200, 64, 256, True, True), (2, 300, 128, 512, False, False)])
def test_gemm_ln_bwd(dev, dtype, G, M, N, K, res, dy2):
    """cmx_gemm_ln_bwd: the LayerNorm backward in the epilogue of the dgrad that produces its input
    (Block.norm2 -> fc1).  dx and the DropPath-scaled dxs are bit-identical to the separate path
    (cmx_gemm dgrad stored in the 16-bit type, then cmx_layernorm_bwd_res), and the per-tile
    dgamma / dbeta partials sum to that kernel's column sums (fp32, another grouping)."""
    from rgbx_semantic_segmentation_amd import kernels as Kk
    torch.manual_seed(2)
    dz = torch.randn(G, M, K, device="cuda").to(dtype)
    W = (torch.randn(G, K, N, device="cuda") / math.sqrt(K)).to(dtype)        # (out = K, in = N)
    x = (torch.randn(G, M, N, device="cuda") * 2 + 0.5).to(dtype)
    gamma = torch.rand(G, N, device="cuda") + 0.5
    beta = torch.randn(G, N, device="cuda")
    _, mean, rstd = Kk.layernorm_fwd(x, gamma, beta, 1e-6, G=G)
    dres = torch.randn(G, M, N, device="cuda").to(dtype) if res else None
    d2 = torch.randn(G, M, N, device="cuda").to(dtype) if dy2 else None
    rps = max(1, M // 2)
    sc = torch.rand(G * M // rps, device="cuda") + 0.5
    dxs = torch.empty_like(x)
    out = Kk.gemm_ln_bwd(dz, W, x, gamma, mean, rstd, dres=dres, dy2=d2, sscale=sc, rows_per_sample=rps, dxs=dxs)
    assert out is not None, "gemm_ln_bwd refused an eligible problem"
    dx, part = out
    # the separate path
    dy = torch.empty_like(x)
    Kk.gemm(dz, W.transpose(1, 2), dy)
    dx0, dxs0 = torch.empty_like(x), torch.empty_like(x)
    nbytes = Kk.query("cmx_layernorm_bwd_workspace", M, G, N, Kk.dtype_code(x))
    ws = Kk._ws(nbytes, x.device)
    gg = torch.zeros(G, N, device="cuda")
    bg = torch.zeros(G, N, device="cuda")
    Kk.call("cmx_layernorm_bwd_res", Kk.ptr(dy), Kk.ptr(d2), Kk.ptr(x), Kk.ptr(gamma), Kk.ptr(mean), Kk.ptr(rstd),
            Kk.ptr(dres), Kk.ptr(sc), Kk.ptr(dxs0), Kk.ptr(dx0), Kk.ptr(gg), Kk.ptr(bg), Kk.ptr(ws), M, G, N, rps, 0,
            Kk.dtype_code(x), Kk.stream())
    torch.cuda.synchronize()
    if N <= 64 or G * ((M + 63) // 64) * 2 > 512:
        assert torch.equal(dx, dx0) and torch.equal(dxs, dxs0)
    else:
        # a small N = 128 grid: the separate dgrad runs 64 x 64 k-group blocks (two k-groups summed
        # at the end) where the fused launch runs one 64 x 128 tile over k in order, so dy -- and dx
        # -- may differ by a rounding
        ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
        for a, b in ((dx, dx0), (dxs, dxs0)):
            assert (a.float() - b.float()).abs().max().item() <= 4 * ulp * b.float().abs().max().item()
    ps = part.double().sum(1)
    assert torch.allclose(ps[:, :N], gg.double(), rtol=1e-4, atol=1e-3 * gg.abs().max().item())
    assert torch.allclose(ps[:, N:], bg.double(), rtol=1e-4, atol=1e-3 * bg.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("G,NIg,H,W,C,R,N,dy2", [(2, 2, 120, 160, 64, 8, 64, True), (2, 2, 60, 80, 128, 4, 128, True),
                                                 (1, 3, 16, 24, 64, 8, 64, False), (2, 1, 20, 12, 128, 4, 128, True)])
def test_conv_patch_dgrad_ln_bwd(dev, dtype, G, NIg, H, W, C, R, N, dy2):
    """cmx_conv_patch_dgrad_ln_bwd: Attention.sr's input gradient (col2im of dy W in the epilogue)
    carried straight into norm1's backward (dy2 = the q projection's gradient of the same norm
    output).  dx / dxs bit-identical to cmx_conv_patch_dgrad + cmx_layernorm_bwd_res; the per-tile
    dgamma / dbeta partials sum to that kernel's column sums."""
    from rgbx_semantic_segmentation_amd import kernels as Kk
    torch.manual_seed(3)
    Ho, Wo = H // R, W // R
    M = NIg * Ho * Wo
    dy = torch.randn(G, M, N, device="cuda").to(dtype)
    Wt = (torch.randn(G, N, R * R * C, device="cuda") / math.sqrt(N)).to(dtype)
    x = (torch.randn(G * NIg, H, W, C, device="cuda") * 2 + 0.5).to(dtype)
    gamma = torch.rand(G, C, device="cuda") + 0.5
    beta = torch.randn(G, C, device="cuda")
    _, mean, rstd = Kk.layernorm_fwd(x, gamma, beta, 1e-6, G=G)
    dres = torch.randn_like(x, dtype=torch.float32).to(dtype)
    d2 = torch.randn_like(x, dtype=torch.float32).to(dtype) if dy2 else None
    rps = H * W
    sc = torch.rand(G * NIg, device="cuda") + 0.5
    dxs = torch.empty_like(x)
    out = Kk.conv_patch_dgrad_ln_bwd(dy, Wt, (G, NIg, H, W, C, R, Ho, Wo), x, gamma, mean, rstd, dres=dres, dy2=d2,
                                     sscale=sc, rows_per_sample=rps, dxs=dxs)
    assert out is not None, "conv_patch_dgrad_ln_bwd refused an eligible problem"
    dx, part = out
    dyc = torch.empty_like(x)
    Kk.call("cmx_conv_patch_dgrad", Kk.ptr(dy), Kk.ptr(Wt), Kk.ptr(dyc), G, NIg, H, W, C, R, Ho, Wo, N, dy.stride(0),
            Wt.stride(0), NIg * H * W * C, Kk.dtype_code(dy), Kk.stream())
    Rr = NIg * H * W
    dx0, dxs0 = torch.empty_like(x), torch.empty_like(x)
    ws = Kk._ws(Kk.query("cmx_layernorm_bwd_workspace", Rr, G, C, Kk.dtype_code(x)), x.device)
    gg = torch.zeros(G, C, device="cuda")
    bg = torch.zeros(G, C, device="cuda")
    Kk.call("cmx_layernorm_bwd_res", Kk.ptr(dyc), Kk.ptr(d2), Kk.ptr(x), Kk.ptr(gamma), Kk.ptr(mean), Kk.ptr(rstd),
            Kk.ptr(dres), Kk.ptr(sc), Kk.ptr(dxs0), Kk.ptr(dx0), Kk.ptr(gg), Kk.ptr(bg), Kk.ptr(ws), Rr, G, C, rps, 0,
            Kk.dtype_code(x), Kk.stream())
    torch.cuda.synchronize()
    assert torch.equal(dx, dx0) and torch.equal(dxs, dxs0)
    ps = part.double().sum(1)
    assert torch.allclose(ps[:, :C], gg.double(), rtol=1e-4, atol=1e-3 * gg.abs().max().item())
    assert torch.allclose(ps[:, C:], bg.double(), rtol=1e-4, atol=1e-3 * bg.abs().max().item())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("G,M,N,K,tB,epi", [(2, 38400, 64, 64, 0, "plain"), (2, 38400, 256, 64, 1, "plain"),
                                            (2, 38400, 64, 256, 0, "res"), (2, 9600, 512, 128, 0, "gelu"),
                                            (1, 99999, 72, 200, 1, "res"), (2, 38400, 64, 64, 0, "fp32"),
                                            (2, 38400, 256, 64, 0, "mask")])
def test_gemm_stream(dev, dt, G, M, N, K, tB, epi):
    """Tall 64 x 64 problems of >= CMX_GEMM_STREAM tiles run on the resident streaming grid
    (gemm_stream_kernel: the LDS ring crosses tile boundaries).  Each tile's k-loop and epilogue
    are the one-tile kernel's, so the result is bit-identical to the one-tile launch of the same
    problem (the knob switched off for one call); ragged M / N / K, every epilogue kind."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    torch.manual_seed(9)
    A = torch.randn(G, M, K, device="cuda").to(dt)
    B = (torch.randn(G, N, K, device="cuda") / math.sqrt(K)).to(dt)
    Bv = B.transpose(1, 2).contiguous().transpose(1, 2) if tB else B
    kw = {}
    if epi == "gelu":
        kw = dict(bias=torch.randn(G, N, device="cuda"), act="gelu")
    if epi in ("res", "mask"):
        kw = dict(bias=torch.randn(G, N, device="cuda"), residual=torch.randn(G, M, N, device="cuda").to(dt),
                  rscale=torch.rand(G * M, device="cuda") + 0.5, rows_per_sample=1)   # one scale per row
    if epi == "mask":
        kw["mask"] = (torch.randn(G, M, N, device="cuda") > 0).to(dt)
    out_dt = torch.float32 if epi == "fp32" else dt
    om = 1 if epi == "fp32" else 0
    C = torch.empty(G, M, N, device="cuda", dtype=out_dt)
    C0 = torch.empty_like(C)
    Kn.gemm(A[:, :64], Bv, C[:, :64], out_mode=om)          # (registers the knob)
    base, base_k = Kn.tune_get("GEMM_STREAM"), Kn.tune_get("GEMM_STREAM_K")
    try:
        Kn.tune("GEMM_STREAM", 256)                          # every shape here on the streaming grid
        Kn.tune("GEMM_STREAM_K", 4096)
        Kn.gemm(A, Bv, C, out_mode=om, **kw)
        Kn.tune("GEMM_STREAM", 0)                            # ... and on one block per tile
        Kn.gemm(A, Bv, C0, out_mode=om, **kw)
    finally:
        Kn.tune("GEMM_STREAM", base)
        Kn.tune("GEMM_STREAM_K", base_k)
    torch.cuda.synchronize()
    assert torch.equal(C, C0)
    ref = torch.bmm(A.float(), B.float().transpose(1, 2))
    if epi == "plain" or epi == "fp32":
        assert rel(C, ref) < (1e-5 if epi == "fp32" else 1e-2)
