"""Sliding-window attention kernels (mi_op_paged_attn_decode_sw / mi_op_paged_attn_prefill_sw) against fp64 softmax
attention over the pool's values with the mask p - W < k <= p; W >= every key: bit-equal to the unwindowed entry points."""

import math

import pytest
import torch

import vllm_neuron_amd._native as lib
from tests.helpers import pool_to_native

pytestmark = pytest.mark.gpu
K_SCALE, V_SCALE = 0.25, 0.5
SHAPES = [(128, 8, 2), (64, 4, 4)]      # hd, nh, nkv: G = 4 and G = 1


def ref_window(q, K, V, q_pos, W):
    """q [T, nh, hd], K / V [S, nkv, hd], q_pos [T] -> [T, nh * hd], all fp64; key k is live iff q_pos - W < k <= q_pos"""
    G, kpos = q.shape[1] // K.shape[1], torch.arange(K.shape[0])
    s = torch.einsum("thd,jhd->htj", q, K.repeat_interleave(G, 1)) / math.sqrt(q.shape[2])
    dead = (kpos[None] > q_pos[:, None]) | (kpos[None] <= q_pos[:, None] - W)
    p = torch.softmax(s.masked_fill(dead[None], float("-inf")), -1)
    return torch.einsum("htj,jhd->thd", p, V.repeat_interleave(G, 1)).reshape(q.shape[0], -1)


def make_pool(f8, nb, bs, nkv, hd, seed):
    """-> (device pool in the native layout, the values it holds as K, V [nb, bs, nkv, hd] fp64)"""
    g = torch.Generator().manual_seed(seed)
    k, v = (torch.randn(nb * bs, nkv, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    if not f8:
        return pool_to_native(k, v, nb, bs).cuda(), k.double().reshape(nb, bs, nkv, hd), v.double().reshape(nb, bs, nkv, hd)
    pool = torch.zeros(2, nb, nkv, bs, hd, dtype=torch.uint8, device="cuda")
    kd, vd, sd = k.cuda(), v.cuda(), torch.arange(nb * bs).cuda()
    lib.check(lib.load_library().mi_op_kv_write_f8(kd.data_ptr(), vd.data_ptr(), sd.data_ptr(), nb * bs, nkv, hd, pool.data_ptr(),
                                                   nb, bs, K_SCALE, V_SCALE, None))
    torch.cuda.synchronize()
    codes = pool.cpu().view(torch.float8_e4m3fn).double().permute(0, 1, 3, 2, 4)          # [2][nb][bs][nkv][hd]
    return pool, codes[0] * K_SCALE, codes[1] * V_SCALE


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
@pytest.mark.parametrize("bs", [16, 32])
@pytest.mark.parametrize("W,ctx", [(1, [1, 2, 33, 65]), (33, [33, 34, 95, 200]), (64, [64, 65, 128, 129]),
                                   (100, [99, 100, 1000, 1031]), (1031, [99, 100, 1000, 1031])])
def test_decode_window(f8, hd, nh, nkv, bs, W, ctx):
    B, MB = len(ctx), (max(ctx) + bs - 1) // bs + 2
    nb = 1 + B * MB
    pool, kk, vv = make_pool(f8, nb, bs, nkv, hd, 4)
    perm = (torch.randperm(nb - 1, generator=torch.Generator().manual_seed(5)) + 1).tolist()
    bt = torch.full((B, MB), -1, dtype=torch.int32)        # pad -1: never read as a block id
    for b in range(B):
        nblk = (ctx[b] + bs - 1) // bs
        bt[b, :nblk] = torch.tensor(perm[b * MB:b * MB + nblk], dtype=torch.int32)
    q = torch.randn(B, nh, hd, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    out, plain = (torch.empty(B, nh * hd, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    L = lib.load_library()
    scratch = torch.empty(L.mi_op_attn_scratch_bytes(B, nh, hd), dtype=torch.uint8, device="cuda")
    qd, btd, cd = q.cuda(), bt.cuda(), torch.tensor(ctx, dtype=torch.int32).cuda()
    head = (qd.data_ptr(), pool.data_ptr(), nb, bs, btd.data_ptr(), MB, cd.data_ptr(), B, nh, nkv, hd)
    lib.check(L.mi_op_paged_attn_decode_sw(*head, int(f8), K_SCALE, V_SCALE, W, out.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    for b, idx in enumerate(map(torch.arange, ctx)):
        blk = bt[b, idx // bs].long()
        ref = ref_window(q[b:b + 1].double(), kk[blk, idx % bs], vv[blk, idx % bs], torch.tensor([ctx[b] - 1]), W)[0]
        err = (out[b].cpu().double() - ref).abs().max().item()
        assert err < 0.02, (b, ctx[b], err)      # the unwindowed decode bar: the same rounding points, fewer keys
    if W >= max(ctx):                            # the window covers every key: the unwindowed kernel's bits
        if f8:
            lib.check(L.mi_op_paged_attn_decode_f8(*head, K_SCALE, V_SCALE, plain.data_ptr(), scratch.data_ptr(), None))
        else:
            lib.check(L.mi_op_paged_attn_decode(*head, plain.data_ptr(), scratch.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(out, plain)


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
@pytest.mark.parametrize("T,pos0,W,bs", [(96, 0, 1, 32), (70, 0, 33, 16), (64, 0, 64, 32), (130, 37, 100, 32), (200, 300, 48, 16),
                                         (33, 0, 200, 32)])
def test_prefill_window(hd, nh, nkv, T, pos0, W, bs):
    kv_len = pos0 + T
    nblk = (kv_len + bs - 1) // bs
    MB, nb = nblk + 2, nblk + 3
    pool, kk, vv = make_pool(False, nb, bs, nkv, hd, 7)
    bt = torch.zeros(MB, dtype=torch.int32)
    bt[:nblk] = (torch.randperm(nb - 1, generator=torch.Generator().manual_seed(8)) + 1)[:nblk].int()
    q = torch.randn(T, nh, hd, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    out, plain = (torch.empty(T, nh * hd, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    qd, btd, L = q.cuda(), bt.cuda(), lib.load_library()
    head = (qd.data_ptr(), T, pos0, pool.data_ptr(), nb, bs, btd.data_ptr(), MB, nh, nkv, hd)
    lib.check(L.mi_op_paged_attn_prefill_sw(*head, W, out.data_ptr(), None))
    torch.cuda.synchronize()
    idx = torch.arange(kv_len)
    blk = bt[idx // bs].long()
    ref = ref_window(q.double(), kk[blk, idx % bs], vv[blk, idx % bs], pos0 + torch.arange(T), W)
    err = (out.cpu().double() - ref).abs().max().item()
    assert not out.isnan().any() and err < 0.03, err           # the unwindowed context-encoding bar
    if W >= kv_len:
        lib.check(L.mi_op_paged_attn_prefill(*head, plain.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(out, plain)
