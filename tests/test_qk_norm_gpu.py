"""mi_op_qk_norm_rope_kv (Qwen3: per-head RMSNorm of q and k, RoPE, q buffer + paged KV write) against fp64 torch."""

import pytest
import torch

NB, MAXPOS, EPS = 6, 4096, 1e-6


def quantize(x, scale):   # the FP8 KV write rule (tests/test_kv_fp8_gpu.py)
    return (x.float() * (1 / scale)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [16, 32])
@pytest.mark.parametrize("T", [1, 5, 33])
@pytest.mark.parametrize("nh,nkv", [(4, 2), (7, 1)])
@pytest.mark.parametrize("hd", [64, 128])
def test_qk_norm_rope_kv(hd, nh, nkv, T, bs):
    from vllm_neuron_amd import _native as N
    g = torch.Generator().manual_seed(hd + nh + T + bs)
    qkv = torch.randn(T, nh + 2 * nkv, hd, generator=g)
    qkv[:, 0] *= 1e3                   # a q head far above ...
    qkv[:, nh] *= 1e-3                 # ... and a k head at the level of eps
    qkv[T - 1, nh - 1] = 0             # a padding head: zero weights
    gq, gk = (1 + 0.1 * torch.randn(2, hd, generator=g)).unbind(0)
    pos = torch.randint(0, 4001, (T,), generator=g, dtype=torch.int32)
    slots = (torch.randperm((NB - 1) * bs, generator=g)[:T] + bs).int()      # never block 0
    slots[T // 2] = -1 if T > 1 else slots[0]
    ang = torch.arange(MAXPOS).double()[:, None] * (1e6 ** (-torch.arange(hd // 2).double() * 2 / hd))[None]
    cos, sin = ang.cos().float(), ang.sin().float()
    dev = [t.contiguous().cuda() for t in (qkv, gq, gk, pos, slots, cos, sin)]

    def run(kv_dtype, ks=1.0, vs=1.0):   # -> q [T, nh, hd], pool rows [2][slot][nkv][hd]
        q = torch.empty(T, nh, hd, dtype=torch.bfloat16, device="cuda")
        pool = (torch.full((2, NB, nkv, bs, hd), 0xAB, dtype=torch.uint8, device="cuda") if kv_dtype
                else torch.full((2, NB, nkv, bs, hd), -7.0, dtype=torch.bfloat16, device="cuda"))        # sentinels
        N.check(N.load_library().mi_op_qk_norm_rope_kv(*[t.data_ptr() for t in dev[:5]], T, nh, nkv, hd, EPS,
                                                       dev[5].data_ptr(), dev[6].data_ptr(), q.data_ptr(), pool.data_ptr(),
                                                       NB, bs, kv_dtype, ks, vs, None))
        torch.cuda.synchronize()
        return q.cpu(), pool.cpu().permute(0, 1, 3, 2, 4).reshape(2, NB * bs, nkv, hd)

    q, rows = run(0)
    y = qkv[:, :nh + nkv].double()
    z = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + EPS) * torch.cat([gq.expand(nh, hd), gk.expand(nkv, hd)]).double()
    a, b, c, s = z[..., 0::2], z[..., 1::2], cos[pos.long()].double()[:, None], sin[pos.long()].double()[:, None]
    ref = torch.stack([a * c - b * s, b * c + a * s], -1).reshape(T, nh + nkv, hd)
    live, written = slots >= 0, slots[slots >= 0].long()
    for got, r in ((q.double(), ref[:, :nh]), (rows[0][written].double(), ref[live, nh:])):   # (a NaN fails the comparison)
        assert ((got - r).abs() <= 2.0 ** -8 * r.abs() + 1e-6).all(), (got - r).abs().max().item()   # one bf16 ulp
    assert (q[T - 1, nh - 1] == 0).all()
    assert torch.equal(rows[1][written], qkv[live, nh + nkv:].to(torch.bfloat16))     # V: rounded, nothing else
    untouched = torch.ones(NB * bs, dtype=torch.bool)
    untouched[written] = False
    assert (rows[:, untouched] == -7.0).all()                                         # the -1 token wrote nothing
    for ks, vs in ((1.0, 1.0), (0.25, 0.5)):
        q8, codes = run(1, ks, vs)
        want = torch.stack([quantize(rows[0], ks), quantize(rows[1], vs)])
        want[:, untouched] = 0xAB
        assert torch.equal(q8, q) and torch.equal(codes, want)
