"""FP8 (e4m3) paged KV on the MI355X: kernels against the rule in torch / fp64 attention, model against the oracle, plugin."""

import pytest
import torch

from tests.helpers import pool_to_native, ref_attention

pytestmark = pytest.mark.gpu

K_SCALE, V_SCALE = 0.25, 0.5


@pytest.fixture(scope="module")
def lib():
    from vllm_neuron_amd import _native
    return _native


def quantize(x, scale):
    """The write rule: bf16 value * (1 / scale) in fp32, clamp, round-nearest-even to e4m3 -> codes (uint8)."""
    return (x.float() * (1 / scale)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def code_pool(nb, bs, nkv, hd, seed, ks=K_SCALE, vs=V_SCALE):
    """-> (device byte pool in the native layout, dequantised K, V as [nb, bs, nkv, hd] fp32)"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(nb * bs, nkv, hd, generator=g).to(torch.bfloat16)
    v = torch.randn(nb * bs, nkv, hd, generator=g).to(torch.bfloat16)
    kc, vc = quantize(k, ks), quantize(v, vs)
    deq = [c.view(torch.float8_e4m3fn).float().reshape(nb, bs, nkv, hd) * s for c, s in ((kc, ks), (vc, vs))]
    return pool_to_native(kc, vc, nb, bs).cuda(), deq[0], deq[1]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.25, 0.5)])
def test_kv_write_f8_bit_exact(lib, hd, ks, vs):
    nb, bs, nkv, T = 6, 32, 2, 40
    g = torch.Generator().manual_seed(3)
    k = (torch.randn(T, nkv, hd, generator=g) * 3).to(torch.bfloat16)
    v = (torch.randn(T, nkv, hd, generator=g) * 3).to(torch.bfloat16)
    k[3, 0, 5], v[7, nkv - 1, hd - 1] = 448 * ks * 2, -448 * vs * 3      # beyond the clamp
    slots = torch.randperm((nb - 1) * bs, generator=g)[:T] + bs          # never block 0
    slots[5] = -1
    pool = torch.zeros(2, nb, nkv, bs, hd, dtype=torch.uint8, device="cuda")
    kd, vd, sd = k.cuda(), v.cuda(), slots.long().cuda()
    lib.check(lib.load_library().mi_op_kv_write_f8(kd.data_ptr(), vd.data_ptr(), sd.data_ptr(), T, nkv, hd,
                                                   pool.data_ptr(), nb, bs, ks, vs, None))
    torch.cuda.synchronize()
    kc, vc = quantize(k, ks), quantize(v, vs)
    assert kc[3, 0, 5] == 0x7E and vc[7, nkv - 1, hd - 1] == 0xFE        # +-448, not the NaN code
    ref = torch.zeros(2, nb, nkv, bs, hd, dtype=torch.uint8)
    for t in range(T):
        s = int(slots[t])
        if s >= 0:
            ref[0, s // bs, :, s % bs] = kc[t]
            ref[1, s // bs, :, s % bs] = vc[t]
    assert torch.equal(pool.cpu(), ref)                                   # untouched rows stay zero


# every tile edge of either tile size; split + combine; 33 sequences x 4 kv heads take the one-launch form
@pytest.mark.parametrize("hd,nh,nkv", [(128, 8, 2), (64, 7, 1), (128, 4, 4)])
@pytest.mark.parametrize("ctx,bs", [([1, 31, 32, 33, 63, 64, 65], 32), ([700, 5, 1024, 257], 32), ([4100, 63, 5000], 32),
                                    ([700, 5, 1024, 257], 16), ([1 + (37 * i) % 200 for i in range(33)], 32)])
def test_paged_attn_decode_f8(lib, hd, nh, nkv, ctx, bs):
    B, MB = len(ctx), (max(ctx) + bs - 1) // bs + 2
    nb = 1 + B * MB
    pool, kk, vv = code_pool(nb, bs, nkv, hd, 4)
    perm = (torch.randperm(nb - 1, generator=torch.Generator().manual_seed(5)) + 1).tolist()
    bt = torch.full((B, MB), -1, dtype=torch.int32)        # pad -1: never read as a block id
    for b in range(B):
        nblk = (ctx[b] + bs - 1) // bs
        bt[b, :nblk] = torch.tensor(perm[b * MB:b * MB + nblk], dtype=torch.int32)
    q = torch.randn(B, nh, hd, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    out = torch.empty(B, nh * hd, dtype=torch.bfloat16, device="cuda")
    scratch = torch.empty(lib.load_library().mi_op_attn_scratch_bytes(B, nh, hd), dtype=torch.uint8, device="cuda")
    qd, btd, cd = q.cuda(), bt.cuda(), torch.tensor(ctx, dtype=torch.int32).cuda()
    lib.check(lib.load_library().mi_op_paged_attn_decode_f8(qd.data_ptr(), pool.data_ptr(), nb, bs, btd.data_ptr(), MB,
                                                            cd.data_ptr(), B, nh, nkv, hd, K_SCALE, V_SCALE,
                                                            out.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    for b in range(B):
        idx = torch.arange(ctx[b])
        blk = bt[b, idx // bs].long()
        ref = ref_attention(q[b:b + 1].double(), kk[blk, idx % bs].double(), vv[blk, idx % bs].double(),
                            torch.tensor([ctx[b] - 1]))
        err = (out[b].cpu().double() - ref[0]).abs().max().item()
        assert err < 0.02, (b, ctx[b], err)      # the bf16 kernel's bar: the conversion adds no error term


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("T,pos0,bs", [(79, 0, 32), (70, 70, 32), (33, 31, 16), (130, 96, 48)])
def test_kv_dequant_gather_then_prefill(lib, hd, T, pos0, bs):
    nh, nkv = 4, 2
    kv_len = pos0 + T
    nblk = (kv_len + bs - 1) // bs
    MB, nb = nblk + 2, nblk + 3
    pool, kk, vv = code_pool(nb, bs, nkv, hd, 7)
    bt = torch.full((MB,), -1, dtype=torch.int32)
    bt[:nblk] = (torch.randperm(nb - 1, generator=torch.Generator().manual_seed(8)) + 1)[:nblk].int()
    staged = torch.empty(2, nblk, nkv, bs, hd, dtype=torch.bfloat16, device="cuda")
    btd = bt.cuda()
    lib.check(lib.load_library().mi_op_kv_dequant_gather(pool.data_ptr(), nb, bs, btd.data_ptr(), MB, kv_len, nkv, hd,
                                                         K_SCALE, V_SCALE, staged.data_ptr(), None))
    torch.cuda.synchronize()
    sel = bt[:nblk].long()
    want = torch.stack([kk[sel], vv[sel]]).permute(0, 1, 3, 2, 4).to(torch.bfloat16)   # [2][nblk][nkv][bs][hd]
    assert torch.equal(staged.cpu(), want)
    # the unchanged context-encoding kernel on the staged pool, identity block table
    q = torch.randn(T, nh, hd, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    out = torch.empty(T, nh * hd, dtype=torch.bfloat16, device="cuda")
    qd, ident = q.cuda(), torch.arange(nblk, dtype=torch.int32).cuda()
    lib.check(lib.load_library().mi_op_paged_attn_prefill(qd.data_ptr(), T, pos0, staged.data_ptr(), nblk, bs,
                                                          ident.data_ptr(), nblk, nh, nkv, hd, out.data_ptr(), None))
    torch.cuda.synchronize()
    idx = torch.arange(kv_len)
    blk = sel[idx // bs]
    ref = ref_attention(q.double(), kk[blk, idx % bs].double(), vv[blk, idx % bs].double(), pos0 + torch.arange(T))
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 0.03, err     # the project's bar for this op (P is rounded to bf16 before the P.V MFMA)


class Fp8KV:
    """The oracle's `kv` tensor with the FP8 write rule applied on the way in (key[1]: 0 = K, 1 = V)."""

    def __init__(self, kv, k_scale, v_scale):
        self.kv, self.scale = kv, (k_scale, v_scale)

    def __getitem__(self, key):
        return self.kv[key]

    def __setitem__(self, key, x):
        s = self.scale[key[1]]
        self.kv[key] = quantize(x, s).view(torch.float8_e4m3fn).float() * s


def fp8_kv_model(cfg, w, ks, vs, artifacts=None):
    from vllm_neuron_amd._native import MI_KV
    from tests import test_model_gpu as T
    import vllm_neuron_amd._native as N
    scales = {f"model.layers.{l}.self_attn.{n}_scale": torch.tensor(s) for l in range(cfg.num_layers) for n, s in (("k", ks), ("v", vs))}
    orig = N.NativeModel
    N.NativeModel = lambda **kw: orig(kv_cache_dtype=MI_KV["fp8"], **kw)     # native_model() builds the config; add the one field
    try:
        return T.native_model(cfg, {**w, **scales}, "bf16", artifacts=artifacts)
    finally:
        N.NativeModel = orig


@pytest.mark.parametrize("name", ["llama31_like", "qwen25_like", "tinyllama_like"])
@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.25, 0.5)])
def test_model_fp8_kv_matches_oracle(name, ks, vs, tmp_path):
    """Device against PagedDecoderOracle(compute="bf16") with the write rule on its KV.  Bar 0.06, the project's
    device-vs-oracle bar.  Measured on an MI355X: 0.050 / 0.051 / 0.052 at scales (1, 1) and
    0.058 / 0.057 / 0.051 at (0.25, 0.5) for llama31_like / qwen25_like / tinyllama_like: the bar is not raised."""
    from oracle import PagedDecoderOracle
    from oracle.synth import make_prompts, make_weights, zoo_config
    from tests.test_model_gpu import BS, NB, load_golden, native_model, scenario
    cfg = zoo_config(name)
    w = make_weights(cfg, seed=1)
    gen, _, _ = load_golden(name)
    prompts = make_prompts(cfg.vocab_size, 0)
    model = fp8_kv_model(cfg, w, ks, vs)
    ref16 = native_model(cfg, w, "bf16")
    assert model.kv_bytes_per_block() * 2 == ref16.kv_bytes_per_block()
    ref16.close()
    oracle = PagedDecoderOracle(cfg, w, NB, BS, compute="bf16")
    oracle.kv = Fp8KV(oracle.kv, ks, vs)
    steps, worst = [], 0.0
    for kind, inp, rows in scenario(prompts, gen):
        got, ref = model.forward(**inp), oracle.forward(**inp)
        steps.append((inp, got.clone()))
        worst = max(worst, (got - ref).abs().max().item())
    print(f"{name} scales ({ks}, {vs}): max |device - oracle| = {worst:.4f}")
    assert worst < 0.06, worst
    model.save_artifacts(str(tmp_path))
    model.close()
    again = fp8_kv_model(cfg, w, ks, vs, artifacts=str(tmp_path))   # the scales survive the round trip: bit-identical logits
    for inp, got in steps:
        assert torch.equal(again.forward(**inp), got)
    again.close()


def test_engine_fp8_kv_matches_golden():
    """kv_cache_dtype="fp8" through the plugin: tokens equal the golden's up to the first step whose golden top-2 gap is
    <= 0.3 (the project's 0.15 plus twice the 0.10 that FP8 KV moves a logit on these weights)."""
    from safetensors import safe_open
    from oracle.synth import make_prompts, make_weights, zoo_config
    from tests.test_engine_gpu import GOLD, hf_like
    from vllm_neuron_amd._vllm_compat import SamplingParams
    from vllm_neuron_amd.engine import MI355XEngine
    name = "tinyllama_like"
    cfg = zoo_config(name)
    eng = MI355XEngine(hf_like(name), max_model_len=256, max_num_seqs=4, block_size=32, kv_cache_dtype="fp8",
                       override_mi355x_config={"state_dict": make_weights(cfg, 1)})
    assert eng.worker.get_kv_cache_spec()["layer"].dtype == torch.float8_e4m3fn
    outs = eng.generate(make_prompts(cfg.vocab_size, 0), SamplingParams(temperature=0.0, max_tokens=12))
    f = safe_open(GOLD, "pt")
    for i, o in enumerate(outs):
        gen, logits = f.get_tensor(f"{name}.generated.{i}").tolist(), f.get_tensor(f"{name}.logits.{i}")
        for s, (a, b) in enumerate(zip(o.token_ids, gen)):
            top2 = logits[s].topk(2).values
            if top2[0] - top2[1] <= 0.3:
                break
            assert a == b, (i, s, a, b)
    eng.worker.model_runner.model.model.close()
