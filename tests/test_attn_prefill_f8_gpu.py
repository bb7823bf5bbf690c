"""Context encoding straight from the FP8 (e4m3) pool: mi_op_paged_attn_prefill_f8 against fp64 attention over
float(code) * scale, the deferred-rescale branch, and chunked against one-call context encoding of an FP8-KV context."""

import pytest
import torch

from tests.helpers import prefill_inputs, ref_attention
from tests.test_kv_fp8_gpu import code_pool, fp8_kv_model, quantize

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from vllm_neuron_amd import _native
    return _native


def run_op(lib, q, T, pos0, pool, nb, bs, bt, nh, nkv, hd, ks, vs):
    out = torch.empty(T, nh * hd, dtype=torch.bfloat16, device="cuda")
    qd, btd = q.cuda(), bt.cuda()
    lib.check(lib.load_library().mi_op_paged_attn_prefill_f8(qd.data_ptr(), T, pos0, pool.data_ptr(), nb, bs, btd.data_ptr(),
                                                             bt.numel(), nh, nkv, hd, ks, vs, out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().double()


def scattered_table(kv_len, bs, seed, extra=2):
    """-> (nb, block table [nblk + extra] padded with -1: never read as a block id)"""
    nblk = (kv_len + bs - 1) // bs
    nb = nblk + 3
    bt = torch.full((nblk + extra,), -1, dtype=torch.int32)
    bt[:nblk] = (torch.randperm(nb - 1, generator=torch.Generator().manual_seed(seed)) + 1)[:nblk].int()
    return nb, bt


# G 4 / 7 / 1 / 8: both piece maps (8 + 8 pieces at head_dim 128, 4 + 4 at 64), an idle head slot, two passes per work-group
@pytest.mark.parametrize("hd,nh,nkv", [(128, 8, 2), (64, 7, 1), (128, 2, 2), (64, 8, 1)])
# less than a tile; exact tile and block edges; a prefix; one query; blocks of one 16-key piece; block 48; more tiles than stages
@pytest.mark.parametrize("T,pos0,bs", [(6, 0, 32), (64, 0, 32), (65, 63, 32), (70, 70, 32), (1, 200, 32), (33, 31, 16),
                                       (130, 96, 48), (300, 0, 32)])
@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.25, 0.5), (0.3, 0.7)])   # the last pair: the folded scale is not the staged value
def test_paged_attn_prefill_f8(lib, hd, nh, nkv, T, pos0, bs, ks, vs):
    kv_len = pos0 + T
    nb, bt = scattered_table(kv_len, bs, 8)
    pool, kk, vv = code_pool(nb, bs, nkv, hd, 7, ks, vs)
    q = torch.randn(T, nh, hd, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    out = run_op(lib, q, T, pos0, pool, nb, bs, bt, nh, nkv, hd, ks, vs)
    idx = torch.arange(kv_len)
    blk = bt[idx // bs].long()
    ref = ref_attention(q.double(), kk[blk, idx % bs].double(), vv[blk, idx % bs].double(), pos0 + torch.arange(T))
    err = (out - ref).abs().max().item()
    assert err < 0.03, err     # the project's bar for this op (P is rounded to bf16; the widening adds no error term)


# G 4 with two blocks per work-group; Gp 8 with an idle head slot and two passes; G 1
@pytest.mark.parametrize("hd,nh,nkv", [(128, 8, 2), (64, 7, 1), (128, 2, 2)])
# tile and block edges plus a prefix; a block size that is no power of two; more tiles than ring stages
@pytest.mark.parametrize("T,pos0,bs", [(65, 63, 32), (130, 96, 48), (300, 0, 32)])
@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.25, 0.5)])
def test_prefill_f8_native_equals_staged_bits(lib, hd, nh, nkv, T, pos0, bs, ks, vs):
    """At power-of-two scales the native kernel and the staged path (mi_op_kv_dequant_gather, then mi_op_paged_attn_prefill
    on the staged copy with an identity table) give the same bits: the two kernels run the same S^T / softmax / P.V step, and scaling every
    K, and separately every V, by a power of two commutes exactly with each fp32 operation and bf16 rounding on the path
    (no value here is near the denormal range)."""
    kv_len = pos0 + T
    nblk = (kv_len + bs - 1) // bs
    nb, bt = scattered_table(kv_len, bs, 8)
    pool, _, _ = code_pool(nb, bs, nkv, hd, 7, ks, vs)
    q = torch.randn(T, nh, hd, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    native = run_op(lib, q, T, pos0, pool, nb, bs, bt, nh, nkv, hd, ks, vs).to(torch.bfloat16)
    staged = torch.empty(2, nblk, nkv, bs, hd, dtype=torch.bfloat16, device="cuda")
    out = torch.empty(T, nh * hd, dtype=torch.bfloat16, device="cuda")
    qd, btd, ident = q.cuda(), bt.cuda(), torch.arange(nblk, dtype=torch.int32).cuda()
    lib.check(lib.load_library().mi_op_kv_dequant_gather(pool.data_ptr(), nb, bs, btd.data_ptr(), bt.numel(), kv_len, nkv,
                                                         hd, ks, vs, staged.data_ptr(), None))
    lib.check(lib.load_library().mi_op_paged_attn_prefill(qd.data_ptr(), T, pos0, staged.data_ptr(), nblk, bs,
                                                          ident.data_ptr(), nblk, nh, nkv, hd, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(native, out.cpu())


def test_paged_attn_prefill_f8_rescale_branch(lib):
    """A spiked key late in the context (6 x the query of row T - 3, head 1; codes ~100, far below 448): the deferred
    rescale of the running maximum must fire, with k_scale inside the score scale that decides it."""
    hd, nh, nkv, bs, T, pos0, ks, vs = 128, 8, 2, 32, 1007, 0, 0.25, 0.5
    nb, bt = scattered_table(T, bs, 18, extra=1)
    pool, kk, vv = code_pool(nb, bs, nkv, hd, 17, ks, vs)
    q = torch.randn(T, nh, hd, generator=torch.Generator().manual_seed(19)).to(torch.bfloat16)
    spike_pos = pos0 + T // 2 + 5
    sb, so = int(bt[spike_pos // bs]), spike_pos % bs
    codes = quantize((6 * q[T - 3, 1].float()).to(torch.bfloat16), ks)
    assert int((codes & 0x7F).max()) < 0x7E
    pool[0, sb, 0, so] = codes.cuda()
    kk[sb, so, 0] = codes.view(torch.float8_e4m3fn).float() * ks
    out = run_op(lib, q, T, pos0, pool, nb, bs, bt, nh, nkv, hd, ks, vs)
    idx = torch.arange(T)
    blk = bt[idx // bs].long()
    ref = ref_attention(q.double(), kk[blk, idx % bs].double(), vv[blk, idx % bs].double(), pos0 + idx)
    err = (out - ref).abs()
    assert err.max().item() < 0.03, (err.max().item(), err.argmax().item())
    got = out.reshape(T, nh, hd)[T - 3, 1]     # the spiked row attends almost only to the spiked key
    assert (got - vv[sb, so, 0].double()).abs().max() < 0.05


def test_fp8_kv_model_chunked_prefill_matches_one_call():
    """FP8-KV context, scales (0.25, 0.5): a prompt in two ragged chunks (the second attends to a prefix through its own
    block-table row) gives the logits of one mi_forward call, within the chunked-prefill bar.  Runs the context's
    context-encoding path: the staged one by default, the native kernel under MI355X_ATTN_PREFILL_F8_NATIVE=1 (the
    native kernel lost the timing rule on a late chunk, DESIGN 5, so the staging pool stays and no workspace bound is
    asserted)."""
    from oracle.synth import make_weights, zoo_config
    from tests.test_model_gpu import BS, MAXLEN
    cfg = zoo_config("tinyllama_like")
    model = fp8_kv_model(cfg, make_weights(cfg, seed=1), 0.25, 0.5)
    prompt = torch.randint(0, cfg.vocab_size, (150,), generator=torch.Generator().manual_seed(11)).tolist()
    whole = model.forward(**prefill_inputs(prompt, [1, 2, 3, 4, 5], BS, MAXLEN)).clone()
    blocks = [9, 6, 10, 7, 8]
    for start, end in ((0, 96), (96, 150)):
        pos = list(range(start, end))
        bt = torch.zeros(1, MAXLEN // BS, dtype=torch.long)
        bt[0, :len(blocks)] = torch.tensor(blocks)
        got = model.forward_chunked(torch.tensor(prompt[start:end]), torch.tensor(pos),
                                    torch.tensor([blocks[i // BS] * BS + i % BS for i in pos]), bt,
                                    torch.tensor([end]), torch.tensor([start]))
    model.close()
    worst = (got[0] - whole[0]).abs().max().item()
    print(f"max |two chunks - one call| = {worst:.4f}")
    assert worst <= 0.06, worst
