// Block-layout paged-KV attention (reference K5/K6/K7 of SURVEY.md §2.2: the NxDI
// context-encoding and token-generation attention reached through
// /root/reference/vllm_neuron/worker/neuronx_distributed_model_loader.py:339-348 with the
// block_table / slot_mapping / *_context_lens contract of
// /root/reference/vllm_neuron/worker/neuronx_distributed_model_runner.py:739-832).
//
// Pool layout (library-owned, one per layer and per K/V):
//     [num_blocks][nkv][block_size][hd] bf16
// i.e. one (block, kv-head) tile is a dense block_size*hd*2-byte range (8 KiB at 32 x 128),
// which a wave streams as 1 KiB coalesced reads.  Block 0 is vLLM's null block
// (reference platform.py:150-159): valid memory, never referenced by a live position.
// The FP8 form of the pool (end of this header) is the same index with one-byte e4m3 elements.
#pragma once
#include "mi_common.h"

namespace mi {

constexpr int kAttnMaxSplits = 16;

int attn_decode_splits(int B, int nkv);
size_t attn_scratch_bytes(int B, int nh, int hd);

// q [B, nh, hd] bf16 -> out [B, nh*hd] bf16.  ctx_lens[b] = number of keys (incl. the new one).
int launch_attn_decode(const uint16_t* q, const uint16_t* kpool, const uint16_t* vpool, int block_size,
                       const int32_t* block_table, int MB, const int32_t* ctx_lens, int B, int nh,
                       int nkv, int hd, uint16_t* out, void* scratch, hipStream_t s, bool tickets_zeroed = false,
                       int rows_per_seq = 1, int num_blocks = 0, int window = 0);
// window W > 0 (sliding-window attention): row b attends the keys ctx_lens[b] - W <= k < ctx_lens[b] and the waves walk only
// the tiles the window touches (windowed instantiations: split + combine, no in-launch merge, no early K/V request)
// num_blocks > 0 (blocks of the pool): a wave's first K/V request does not wait for the context length (ids clamped into the pool)
// rows_per_seq R > 1: batch rows b R .. b R + R - 1 are one sequence at consecutive positions (block_table row b R
// serves them all); their heads share the MFMA columns and the sequence's K/V is read once
// tickets_zeroed: the first 4 KiB of `scratch` (the merge tickets) were zeroed once by the owner and
// only ever touched by these launches (which leave them at zero): enables the in-launch merge

// One sequence: q [T, nh, hd] at absolute positions q_pos0.., keys 0..q_pos0+T-1 from the pool.
// A sequence may span at most kPrefillMaxBlocks blocks (131072 tokens at block_size 32): the bound mi_ctx_create holds
// max_model_len to, so every context that exists fits; the kernels themselves read the block table from memory.
constexpr int kPrefillMaxBlocks = 4096;
int launch_attn_prefill(const uint16_t* q, int T, int q_pos0, const uint16_t* kpool,
                        const uint16_t* vpool, int block_size, const int32_t* block_table, int nh,
                        int nkv, int hd, uint16_t* out, hipStream_t s, int window = 0);
// window W > 0: query p attends the keys p - W < k <= p.  q_pos0 + T <= W (the window covers every key) takes the
// unwindowed kernel and launch geometry; otherwise the windowed variant (adjacent query blocks per work-group, the K/V ring
// walks the work-group's band of tiles only)

// k, v [T, nkv, hd] bf16 -> pool at slots [T] (-1 skips)
int launch_kv_write(const uint16_t* k, const uint16_t* v, const int64_t* slots, int T, int nkv, int hd,
                    uint16_t* kpool, uint16_t* vpool, int block_size, hipStream_t s);

// Qwen3: qkv [T, (nh + 2 nkv) * hd] fp32 (the fused projection with EPI_F32: q / k heads pair-interleaved, V plain) ->
// per-head RMSNorm of every q and k head with gains gq / gk [hd] (interleaved like the columns), RoPE, bf16: q to
// q_out [T, nh * hd], k and (un-normalised) v to the pool rows of slots [T] (-1, or a slot outside the pool, skips) --
// the layout and dimension order EPI_QKV / EPI_QKV_F8 write.  f8: byte pools and the kv_quant4 write rule.
// hd 64 or 128; rope_cos / rope_sin [max_pos, hd / 2] must cover every pos.
int launch_qk_norm_rope_kv(const float* qkv, const float* gq, const float* gk, const int32_t* pos, const int32_t* slots,
                           int T, int nh, int nkv, int hd, float eps, const float* rope_cos, const float* rope_sin,
                           uint16_t* q_out, void* kpool, void* vpool, int num_blocks, int block_size, bool f8, float k_scale,
                           float v_scale, hipStream_t s);

// ---- FP8 (OCP e4m3fn) pool: [num_blocks][nkv][block_size][hd] BYTES per K / V, static scales --------------------
// write: code = rne_e4m3(clamp(float(x_bf16) * (1.0f / scale), -448, 448)); read: value = float(code) * scale.
// k, v [T, nkv, hd] bf16 -> byte pool at slots [T] (-1 skips)
int launch_kv_write_f8(const uint16_t* k, const uint16_t* v, const int64_t* slots, int T, int nkv, int hd, uint8_t* kpool,
                       uint8_t* vpool, int block_size, float k_scale, float v_scale, hipStream_t s);
// launch_attn_decode over the byte pool (same grid, splits, scratch layout and combine; no in-launch merge).
// k_scale rides in the score scale, v_scale multiplies the merged output once; every MFMA is bf16.
int launch_attn_decode_f8(const uint16_t* q, const uint8_t* kpool, const uint8_t* vpool, int block_size,
                          const int32_t* block_table, int MB, const int32_t* ctx_lens, int B, int nh, int nkv, int hd,
                          float k_scale, float v_scale, uint16_t* out, void* scratch, hipStream_t s, int rows_per_seq = 1,
                          int num_blocks = 0, int window = 0);
// launch_attn_prefill over the byte pool, read natively (attn_prefill_f8_kernel: codes widened once per work-group in
// LDS, no bf16 copy in memory).  The same shape checks, plus block_size % 16 == 0 and positive scales; k_scale rides in
// the score scale, v_scale multiplies the normalised output once.  No byte of a block the table names for keys
// 0 .. q_pos0 + T - 1 may be the e4m3 NaN code (masking is by score, as for launch_attn_decode_f8).
int launch_attn_prefill_f8(const uint16_t* q, int T, int q_pos0, const uint8_t* kpool, const uint8_t* vpool,
                           int block_size, const int32_t* block_table, int nh, int nkv, int hd, float k_scale,
                           float v_scale, uint16_t* out, hipStream_t s);
// (no windowed variant: a windowed context whose keys outgrow the window takes the staged path whatever the switch says)
// One sequence's blocks 0 .. ceil(kv_len / block_size) - 1, in block-table order, widened to a bf16 pool
// staged [2][nblk][nkv][block_size][hd] (element bf16_rne(float(code) * scale)) that launch_attn_prefill reads with an
// identity block table.  pool: K bytes, then V bytes (num_blocks blocks each).
int launch_kv_dequant_gather(const uint8_t* pool, int num_blocks, int block_size, const int32_t* block_table, int MB,
                             int kv_len, int nkv, int hd, float k_scale, float v_scale, uint16_t* staged, hipStream_t s,
                             int first_blk = 0);
// first_blk > 0 (sliding window): only blocks first_blk .. are widened, into the places they have in the full staged pool

}  // namespace mi
