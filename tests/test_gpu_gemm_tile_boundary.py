"""Tile boundaries of the ping-pong GEMM (csrc/gemm_pp.hip): the walk is a tile loop around a K loop whose first
K-step per tile is an instance of its own (its MFMAs start from a zero C, so the accumulators are never zeroed, and
its counted waits allow for the stores of the epilogue before it), and the head-major store address is computed
once per tile.

All of it is schedule only: every output must equal the interleaved kernel's (gemm_bf16.hip) bit for bit.  The
shapes are the smallest that reach each path: K = 64 (every K-step starts a tile), K = 128 (no steady K-step after
the second), K = 192 / 256 (3 / 4 K-steps per tile), and a ragged shape that puts boundaries which count no stores
next to full tiles.  Every shape has more than four tiles per workgroup on 256 CUs, so several boundaries follow
one another with stores still pending.
"""
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SHAPES = [(12288, 5632, 64), (12288, 5632, 128), (12288, 5632, 192), (12288, 5632, 256), (12100, 5700, 192)]
# the f32 residual epilogue reaches the ping-pong kernel only from K = 2048 (gemm_pingpong_fits): one more shape,
# so that its read-modify-write runs at a tile boundary of this kernel too
RESID_SHAPE = (12288, 5632, 2048)


def _run_pair(M, N, K, epi, aux_rows=192, seed=0):
    """The same GEMM through the interleaved-K-step kernel and the ping-pong kernel (MQ_TUNE_GEMM_PINGPONG, key 12)."""
    import torch
    from mqhip import _lib
    ctx = _lib.Context.get(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    A = torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16)
    W = (torch.randn((N, K), generator=g, device="cuda") * 0.05).to(torch.bfloat16)
    bias = torch.randn((N,), generator=g, device="cuda")
    aux = torch.randn((aux_rows, N), generator=g, device="cuda")
    # The bf16 epilogues store 8 columns (16 bytes) per lane in both kernels and mask a store by its first column, so
    # with N % 8 == 4 a row's last store runs 4 columns over: C then needs rows padded to a multiple of 8 (ldc), or
    # the overrun lands in the next row and races with that row's own tile.  The padding columns are not compared.
    ldc = (N + 7) // 8 * 8 if epi in (0, 1, 6) else N
    C0 = torch.randn((M, ldc), generator=g, device="cuda")
    if epi in (0, 1, 6):
        C0 = C0.to(torch.bfloat16)
    outs = []
    old = ctx.lib.mq_get_tuning(12)
    try:
        for pp in (0, 1):
            assert ctx.lib.mq_set_tuning(12, pp) == 0
            Cm = C0.clone()
            _lib.check(ctx.lib.mq_gemm_bf16(ctx.handle, _lib.ptr(A), _lib.ptr(W), _lib.ptr(Cm), _lib.ptr(bias),
                                            _lib.ptr(aux), M, N, K, K, K, ldc, aux_rows, epi, _lib.stream_ptr()),
                       "mq_gemm_bf16")
            outs.append(Cm[:, :N].contiguous())
    finally:
        ctx.lib.mq_set_tuning(12, old)
    torch.cuda.synchronize()
    return outs


def _assert_same_bits(outs):
    import torch
    bits = [o.view(torch.int16) if o.dtype == torch.bfloat16 else o.view(torch.int32) for o in outs]
    assert torch.equal(bits[0], bits[1])


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 6])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_tile_boundary_bitwise_equals_interleaved(epi, M, N, K):
    _assert_same_bits(_run_pair(M, N, K, epi))


def test_tile_boundary_residual_epilogue_at_pingpong_k():
    _assert_same_bits(_run_pair(*RESID_SHAPE, 2))


def test_tile_boundary_repeated_launches_agree():
    """A wait that retires too little is a race, not a fixed error: the same launch three times must not differ."""
    import torch
    first = _run_pair(12288, 5632, 192, 1)[1]
    for _ in range(2):
        assert torch.equal(_run_pair(12288, 5632, 192, 1)[1].view(torch.int16), first.view(torch.int16))


def test_head_major_qkv_matches_row_major():
    """The qkv GEMM of a ViT-H-wide layer (N = 3840, head_dim 80, M = 64 images x 192 tokens: 2.8 tiles per CU) with
    head-major stores against the row-major layout.  mq_gemm_bf16 does not expose head_dim, so both run inside the
    forward (MQ_TUNE_QKV_HEAD_MAJOR, key 20), where the attention reads the layout that the GEMM wrote: any
    misplaced element changes the heatmaps, which must agree bit for bit."""
    import torch
    from mqhip import _lib
    from mqhip.pose import VitPoseHip
    from mqhip.weights import VitPoseConfig, make_random_weights
    cfg = VitPoseConfig("huge1", 1280, 1, 16, 5120)
    assert cfg.head_dim == 80 and 3 * cfg.embed_dims == 3840
    w = make_random_weights(cfg, seed=5, device="cuda")
    crops = torch.randn((32, 3, 256, 192), device="cuda")
    model = VitPoseHip(cfg, w, graph=False)
    ctx = _lib.Context.get(0)
    old = ctx.lib.mq_get_tuning(20)
    outs = []
    try:
        for hm in (0, 1):
            assert ctx.lib.mq_set_tuning(20, hm) == 0
            outs.append(model.forward(crops).clone())
    finally:
        ctx.lib.mq_set_tuning(20, old)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
