// Paged-KV attention kernels for gfx950.  See attn_kernels.h for the contract.
//
// Token generation (attn_decode_kernel): HBM-bound.  One work-group per
// (context split, kv head, sequence); its waves walk 32-token tiles of the sequence's blocks,
// two tiles in flight per wave.  The query heads of the kv group are the columns of MFMA tiles
// (S^T = K.Q^T from K fragments loaded straight from the pool; O^T += V^T.P^T with V parked in a
// wave-private LDS tile and read transposed), so the arithmetic per byte is a few hundred
// cycles per 16 KiB tile -- the VALU dot-product form this replaced cost ~3000.  With fewer
// (sequence, kv head) pairs than CUs the context is split over work-groups and the splits are
// merged by attn_combine_kernel in a fixed order (deterministic); otherwise one work-group
// covers the whole sequence.
//
// attn_decode_f8_kernel is the same walk over an FP8 (e4m3) pool: 64-token tiles of bytes, codes widened to bf16 in
// registers.
//
// Context encoding (attn_prefill2_kernel over a bf16 pool, attn_prefill_f8_kernel over an FP8 pool): MFMA flash
// attention, one wave per 32-query block of one q head, the waves of a kv group sharing 64-key K/V tiles that LDS-DMA
// brings into a ring in LDS.  Scores are computed transposed (S^T = K.Q^T) so the accumulator registers ARE the B
// operand of the P.V product (no LDS round trip for P); V stays row-major in LDS and is read transposed.  The two
// kernels have the same maps, query-block ownership, S^T / softmax / P.V step and epilogue and differ in how a tile
// reaches its bf16 image in LDS: straight by DMA, or as codes that the work-group widens once.
//
// Sliding window (Mistral): the two token-generation kernels and attn_prefill2_kernel have a windowed instantiation (template
// parameter SW) that walks only the K/V tiles the window touches; the unwindowed instantiations are the code they were.
//
// Also here: the standalone K/V writes into either pool and the FP8 -> bf16 staging gather.

#include <type_traits>

#include "attn_kernels.h"

namespace mi {

#define MI_TRY_A(expr)             \
  do {                             \
    int _rc = (expr);              \
    if (_rc != MI_OK) return _rc;  \
  } while (0)

// LDS-DMA: 64 lanes x 16 bytes from per-lane global addresses into 1 KiB of LDS starting at `l` (wave-uniform)
__device__ __forceinline__ void glds16(const void* g, unsigned char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
// exp2(x - m) with the -inf conventions of online softmax (m finite or -inf)
__device__ __forceinline__ float sexp2(float x, float m) {
  return (x == -INFINITY) ? 0.f : fexp2(x - m);
}

// =====================================================================================
// token generation
// =====================================================================================
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

// NW waves per work-group.  FINAL: the work-group covers the whole context of its (sequence, kv
// head) and writes the bf16 output itself (grid (1, nkv, B)); otherwise it covers context split
// blockIdx.x of NS and leaves (o, m, l) partials for attn_combine_kernel.
//
// A wave walks 32-token tiles.  The G <= 16 query heads of the kv group are the 16 columns of the
// MFMA tiles (the idle columns cost nothing: the kernel is bound by bytes, not by the matrix core):
//     S^T[token][head]  = K_tile . Q^T             2 x HD/32 MFMA 16x16x32 (two 16-token halves)
//     O^T[d][head]     += V_tile^T . P^T           HD/16 MFMA 16x16x32, k = the tile's 32 tokens
// K goes from the pool straight into A fragments (lane (g, c): token c, 16 B of the row).  V is
// read as whole rows, parked row-major in a wave-private LDS tile and picked up transposed by
// ds_read_b64_tr_b16.  The P.V k-slot (g, j) is bound to token (j < 4 ? 4g + j : 16 + 4g + j - 4),
// which is where the two S^T accumulators already hold that token's score, so the exponentiated
// scores are the B operand as they stand.
// Every wave keeps TWO tiles in flight (the next tile is requested before the current one is
// consumed); a tile past the wave's range is requested as one harmless line of the null block, so
// the loop has no predicated loads.  Rows of the last tile beyond the context are masked by score;
// the pool must not hold NaN/Inf there (the library zero-fills it and only ever writes finite values).
//
// MERGE (with !FINAL): the context splits of one (sequence, kv head) are merged by whichever of
// their NS work-groups finishes LAST, inside this launch -- no combine launch.  No work-group ever
// waits for another (nothing can hang): each publishes its partial with write-through (sc1) stores,
// every storing wave drains them, one lane takes a ticket from an agent-scope counter, and the
// work-group whose ticket is NS - 1 reads all NS partials back with sc1 loads (past its L1; no
// other reader of these lines exists in the launch, so no L2 holds a stale copy) and writes the
// bf16 output.  This is the hand-off form MI355X_MICROARCH.md lists as valid without fences
// ("the workgroup whose add came last, told by the value its add returned"; one work-group per
// CU: the launch pads its LDS request to keep it so).  The merge itself runs in split order, so the
// result does not depend on which work-group performs it.  The counter is left at 0 for the next launch.
//
// SW (sliding window W >= 1): column c attends the keys ctx_c - W <= tok < ctx_c.  The waves walk only the tiles the window
// of the sequence touches: t_lo = max(0, min over the R rows of ctx_r - W) / 32 (for R = 1 that is max(0, ctx - W) / 32; with
// R > 1 the row with the SHORTEST context has the lowest edge), dealt round-robin from t_lo on, so wave w of split s starts
// at t_lo + s NW + w.  That tile depends on the context length: no early request.  A column whose first tile holds no live
// key (its edge lies in a later tile than another column's) keeps m = -inf, l = 0 through sexp2's conventions.
template <int HD, int NW, bool FINAL, bool MERGE = false, bool SW = false>
__global__ __launch_bounds__(NW * 64) void attn_decode_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kpool, const uint16_t* __restrict__ vpool,
    int bs, const int32_t* __restrict__ block_table, int MB, const int32_t* __restrict__ ctx_lens,
    int nh, int nkv, int G, int NS, float* __restrict__ o_part, float* __restrict__ ml_part,
    uint16_t* __restrict__ out, float scale_log2e, unsigned int* __restrict__ tickets = nullptr, int R = 1,
    int num_blocks = 0, int window = 0) {
  static_assert(!(SW && MERGE), "the windowed form has no in-launch merge");
  // R > 1 (the target's pass of a speculation step): batch rows b R .. b R + R - 1 are the SAME sequence
  // at consecutive positions (one block-table row, context lengths growing by one).  Their query heads
  // sit side by side in the 16 MFMA columns (column = row-in-sequence * G + head, G R <= 16) and each
  // column masks by its own row's context length: the K/V of the sequence is read once, not R times.
  constexpr int KP = HD + 8;        // LDS row pitch (elements)
  constexpr int CPR = HD / 8;       // 16-byte chunks per row
  constexpr int KS = HD / 32, DN = HD / 16;
  constexpr int NV = 32 * CPR / 64; // 16-byte V loads per lane per tile
  constexpr int VT = 32 * KP;       // elements of one wave's V tile
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  uint16_t* Vs = reinterpret_cast<uint16_t*>(dsm);                       // [NW][32][KP] bf16
  float* sm_ml = reinterpret_cast<float*>(dsm + (size_t)NW * VT * 2);    // [NW][16][2]

  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z * R;   // b: first batch row of the sequence
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int Gc = G * R;                         // live MFMA columns
  const int cr = c / G, ch = c - cr * G;        // column c = (row of the sequence, head of the kv group)
  int ctx = 0;                                  // the longest context of the sequence's rows bounds the tiles walked
  for (int r = 0; r < R; ++r) ctx = max(ctx, ctx_lens[b + r]);
  const int ctx_c = c < Gc ? ctx_lens[b + cr] : 0;   // what this lane's column may attend to
  int t_lo = 0;                                 // SW: the first tile any row's window touches
  if constexpr (SW) {
    int lo = ctx;
    for (int r = 0; r < R; ++r) lo = min(lo, ctx_lens[b + r]);
    t_lo = max(lo - window, 0) / 32;
  }
  const int lo_c = SW ? ctx_c - window : 0;     // SW: the first key of this lane's column
  // Tiles are dealt round-robin: wave w of split s takes tiles s NW + w, + NS NW, ...  Which tile a wave STARTS
  // with therefore does not depend on the context length, so (num_blocks > 0) its first K/V request goes out
  // beside the load of the context length instead of behind it (one L2 round trip less on the way to the first
  // MFMA); what it fetched is masked by score, or never consumed when the tile lies beyond the context.
  const int nt = ceil_div(ctx, 32), stride = NS * NW;
  const int t_first = t_lo + split * NW + wave, t_end = nt;
  uint16_t* Vw = Vs + wave * VT;

  u32x4_t kA[2 * KS], vA[NV], kB[2 * KS], vB[NV];
  // A 32-token tile is two 16-token halves; with block_size 16 (vLLM's default) they sit in two
  // different blocks, so each half looks its own block up (the same block for block_size % 32 == 0).
  auto issue = [&](u32x4_t (&kr)[2 * KS], u32x4_t (&vr)[NV], int tt) {
    const bool live = tt < t_end;
    const int tok0 = live ? tt * 32 : 0;
    size_t rowh[2];   // pool row of the first token of each half
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // the second half of the last tile may lie beyond the context (and beyond the table): masked by score, read from the null block
      const bool in = live && (tok0 + 16 * u) < ctx;
      const int blk = in ? block_table[(size_t)b * MB + (tok0 + 16 * u) / bs] : 0;
      rowh[u] = in ? ((size_t)blk * nkv + kvh) * bs + ((tok0 + 16 * u) % bs) : 0;
    }
    // K fragment (u, ks): token 16u + c, dims 32 ks + 8 g ..
    const size_t kk = live ? 32 : 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t kbase = live ? (rowh[u] + c) * HD + g * 8 : 0;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        kr[u * KS + ks] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(kpool + kbase + ks * kk));
    }
    // V rows: lane-linear 16-byte chunks (whole rows per instruction); load i covers rows
    // [i * 64 / CPR, (i + 1) * 64 / CPR) of the tile, i.e. half (i * 64 / CPR) / 16
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (lane + 64 * i) / CPR, ch = (lane + 64 * i) % CPR;   // row of the tile, 16-byte chunk of the row
      const size_t src = live ? (rowh[row >> 4] + (row & 15)) * HD + ch * 8 : 0;
      vr[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(vpool + src));
    }
  };
  if (!SW && num_blocks > 0) {
    // speculative form of issue(): no use of the context length; table index and block id clamped into range
    const int tok0 = t_first * 32;
    size_t rowh[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int bi = min((tok0 + 16 * u) / bs, MB - 1);
      const int blk = min(max(block_table[(size_t)b * MB + bi], 0), num_blocks - 1);
      rowh[u] = ((size_t)blk * nkv + kvh) * bs + ((tok0 + 16 * u) % bs);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t kbase = (rowh[u] + c) * HD + g * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        kA[u * KS + ks] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(kpool + kbase + ks * 32));
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (lane + 64 * i) / CPR, chn = (lane + 64 * i) % CPR;
      vA[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(vpool + (rowh[row >> 4] + (row & 15)) * HD + chn * 8));
    }
  } else {
    issue(kA, vA, t_first);
  }

  u32x4_t qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = (c < Gc) ? *reinterpret_cast<const u32x4_t*>(q + ((size_t)(b + cr) * nh + kvh * G + ch) * HD + ks * 32 + g * 8)
                      : u32x4_t{0, 0, 0, 0};
  f32x4_t acc[DN];
#pragma unroll
  for (int dn = 0; dn < DN; ++dn) acc[dn] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float mrow = -INFINITY, lrow = 0.f;   // head c: running max (same on its 4 lanes), this lane's share of the sum
  const int tr_row = (lane & 15) >> 2, tr_col = (lane & 3) * 4;

  auto update = [&](const u32x4_t (&kr)[2 * KS], const u32x4_t (&vr)[NV], int tt) {
    // park V (the previous tile's transposed reads are complete: their values fed MFMAs already)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = lane + 64 * i;
      *reinterpret_cast<u32x4_t*>(&Vw[(idx / CPR) * KP + (idx % CPR) * 8]) = vr[i];
    }
    asm volatile("" ::: "memory");   // LDS ops of one wave execute in order; keep the compiler from reordering them
    f32x4_t st[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      st[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const u32x4_t kw = kr[u * KS + ks], qw = qf[ks];
        st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kw), __builtin_bit_cast(bf16x8_t, qw), st[u], 0, 0, 0);
      }
    }
    s16x4_t vlo[DN], vhi[DN];
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) {
      const uint16_t* r0 = &Vw[(4 * g + tr_row) * KP + 16 * dn + tr_col];
      vlo[dn] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)r0);
      vhi[dn] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(r0 + 16 * KP));
    }
    const int tok0 = tt * 32;
    float pv[8];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float sv = st[u][i] * scale_log2e;
        if (tok0 + 16 * u + 4 * g + i >= ctx_c) sv = -INFINITY;
        if constexpr (SW) { if (tok0 + 16 * u + 4 * g + i < lo_c) sv = -INFINITY; }
        pv[4 * u + i] = sv;
        mx = fmaxf(mx, sv);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));       // -inf where the column has no live token in this tile (sexp2 conventions)
    const float mn = fmaxf(mrow, mx);
    const float alpha = sexp2(mrow, mn);
    float ps = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      pv[k] = sexp2(pv[k], mn);
      ps += pv[k];
    }
    const bool moved = mn != mrow;
    mrow = mn;
    lrow = lrow * alpha + ps;
    union { uint32_t w[4]; bf16x8_t v; } pk;
#pragma unroll
    for (int k = 0; k < 4; ++k) pk.w[k] = pack_bf16x2(pv[2 * k], pv[2 * k + 1]);
    if (__any(moved)) {
#pragma unroll
      for (int dn = 0; dn < DN; ++dn) {
        acc[dn][0] *= alpha; acc[dn][1] *= alpha; acc[dn][2] *= alpha; acc[dn][3] *= alpha;
      }
    }
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) {
      const s16x4_t lo = vlo[dn], hi = vhi[dn];
      const bf16x8_t a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      acc[dn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pk.v, acc[dn], 0, 0, 0);
    }
  };

  for (int tt = t_first; tt < t_end; tt += 2 * stride) {
    issue(kB, vB, tt + stride);
    update(kA, vA, tt);
    issue(kA, vA, tt + 2 * stride);
    if (tt + stride < t_end) update(kB, vB, tt + stride);
  }

  // ---- merge the waves: O^T / m / l of wave w go to its own (now idle) LDS tile --------------
  lrow += __shfl_xor(lrow, 16);
  lrow += __shfl_xor(lrow, 32);
  asm volatile("" ::: "memory");
  float* so = reinterpret_cast<float*>(Vw);            // [16 heads][HD] f32 = 8 KiB at HD 128 <= the tile
#pragma unroll
  for (int dn = 0; dn < DN; ++dn) *reinterpret_cast<f32x4_t*>(&so[c * HD + 16 * dn + 4 * g]) = acc[dn];
  if (g == 0) {
    sm_ml[(wave * 16 + c) * 2] = mrow;
    sm_ml[(wave * 16 + c) * 2 + 1] = lrow;
  }
  __syncthreads();
  for (int idx = tid; idx < Gc * HD; idx += NW * 64) {
    const int h = idx / HD, d = idx % HD;       // h: MFMA column
    const int hr = h / G, hh = h - hr * G;      // -> (row of the sequence, head)
    float M = sm_ml[h * 2];
#pragma unroll
    for (int w = 1; w < NW; ++w) M = fmaxf(M, sm_ml[(w * 16 + h) * 2]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {  // wave order: deterministic
      const float f = sexp2(sm_ml[(w * 16 + h) * 2], M);
      o += f * reinterpret_cast<const float*>(Vs + w * VT)[h * HD + d];
      L += f * sm_ml[(w * 16 + h) * 2 + 1];
    }
    if constexpr (FINAL) {
      out[((size_t)(b + hr) * nh + kvh * G + hh) * HD + d] = f32_to_bf16(L > 0.f ? o / L : 0.f);   // empty context -> zeros
    } else if constexpr (MERGE) {
      const size_t row = ((size_t)(b + hr) * nh + kvh * G + hh) * kAttnMaxSplits + split;   // fixed stride: a head's m/l block is one 128-byte line
      __hip_atomic_store(&o_part[row * HD + d], o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // global_store ... sc1
      if (d == 0) {
        __hip_atomic_store(&ml_part[row * 2], M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ml_part[row * 2 + 1], L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      const size_t row = ((size_t)(b + hr) * nh + kvh * G + hh) * kAttnMaxSplits + split;   // fixed stride: a head's m/l block is one 128-byte line
      o_part[row * HD + d] = o;
      if (d == 0) {
        ml_part[row * 2] = M;
        ml_part[row * 2 + 1] = L;
      }
    }
  }
  if constexpr (MERGE && !FINAL) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // EVERY storing wave drains its write-through stores
    __syncthreads();
    int* s_last = reinterpret_cast<int*>(sm_ml);        // the m/l staging is dead behind the barrier
    if (tid == 0) {
      unsigned int* tk = tickets + (size_t)b * nkv + kvh;
      const unsigned int t = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = t == (unsigned int)(NS - 1);
      if (last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
      *s_last = last ? 1 : 0;
    }
    __syncthreads();
    if (*s_last) {
      for (int idx = tid; idx < G * HD; idx += NW * 64) {
        const int h = idx / HD, d = idx % HD;
        const size_t row0 = ((size_t)b * nh + kvh * G + h) * kAttnMaxSplits;
        float mv[kAttnMaxSplits], lv[kAttnMaxSplits], ov[kAttnMaxSplits];
#pragma unroll
        for (int sp = 0; sp < kAttnMaxSplits; ++sp) {
          const bool ok = sp < NS;
          mv[sp] = ok ? __hip_atomic_load(&ml_part[(row0 + sp) * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -INFINITY;
          lv[sp] = ok ? __hip_atomic_load(&ml_part[(row0 + sp) * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
          ov[sp] = ok ? __hip_atomic_load(&o_part[(row0 + sp) * HD + d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        }
        float M = -INFINITY;
#pragma unroll
        for (int sp = 0; sp < kAttnMaxSplits; ++sp) M = fmaxf(M, mv[sp]);
        float acc_o = 0.f, L = 0.f;
#pragma unroll
        for (int sp = 0; sp < kAttnMaxSplits; ++sp) {   // split order: the same sums as attn_combine_kernel
          const float f = sexp2(mv[sp], M);
          acc_o += f * ov[sp];
          L += f * lv[sp];
        }
        out[((size_t)b * nh + kvh * G + h) * HD + d] = f32_to_bf16(L > 0.f ? acc_o / L : 0.f);
      }
    }
  }
}
template <int HD, int NW>
constexpr size_t attn_decode_lds() { return (size_t)NW * 32 * (HD + 8) * 2 + (size_t)NW * 16 * 2 * sizeof(float); }

// Merge the context splits of one (sequence, head) in split order.  All partials are
// fetched before the first use (kAttnMaxSplits is a compile-time bound), so the kernel is
// one L2 round trip deep.
template <int HD>
__global__ __launch_bounds__(HD) void attn_combine_kernel(const float* __restrict__ o_part, const float* __restrict__ ml_part,
                                                          int NS, int nh, uint16_t* __restrict__ out) {
  const int head = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const size_t row0 = ((size_t)b * nh + head) * kAttnMaxSplits;
  float mv[kAttnMaxSplits], lv[kAttnMaxSplits], ov[kAttnMaxSplits];
#pragma unroll
  for (int s = 0; s < kAttnMaxSplits; ++s) {
    const bool ok = s < NS;
    const float2 ml = ok ? *reinterpret_cast<const float2*>(ml_part + (row0 + s) * 2) : make_float2(-INFINITY, 0.f);
    mv[s] = ml.x;
    lv[s] = ml.y;
    ov[s] = ok ? o_part[(row0 + s) * HD + d] : 0.f;
  }
  float M = -INFINITY;
#pragma unroll
  for (int s = 0; s < kAttnMaxSplits; ++s) M = fmaxf(M, mv[s]);
  float acc = 0.f, L = 0.f;
#pragma unroll
  for (int s = 0; s < kAttnMaxSplits; ++s) {
    const float f = sexp2(mv[s], M);
    acc += f * ov[s];
    L += f * lv[s];
  }
  out[((size_t)b * nh + head) * HD + d] = f32_to_bf16(L > 0.f ? acc / L : 0.f);   // empty context -> zeros
}

int attn_decode_splits(int B, int nkv) {
  int ns = 256 / (B * nkv);  // ~one work-group per CU; >= 4 tiles (one per wave) each at 1k context
  return ns < 1 ? 1 : (ns > kAttnMaxSplits ? kAttnMaxSplits : ns);
}
// [tickets: kAttnTickets counters, one per (sequence, kv head), zero between launches]
// [m/l partials: B x nh rows of one 128-byte line][o partials]  -- the ticket block and the m/l
// rows sit at offsets that do not depend on the batch size of the call
constexpr int kAttnTickets = 1024;
size_t attn_scratch_bytes(int B, int nh, int hd) {
  return kAttnTickets * sizeof(unsigned int) + (size_t)B * nh * kAttnMaxSplits * (hd + 2) * sizeof(float);
}
// Off by default: measured on Llama-3.1-8B decode (B 4, ctx 1024) the in-launch merge costs the
// last work-group ~5.4 us (write-through drain + returning atomic + sc1 read-back are three
// dependent trips to memory) against 4.8 us for the separate combine launch: 2.157 vs 2.138 ms per
// step.  MI355X_ATTN_MERGE=1 selects it (same results: tests/test_model_gpu.py runs both).
static bool attn_merge_enabled() {
  static const bool on = [] { const char* v = getenv("MI355X_ATTN_MERGE"); return v && v[0] == '1'; }();
  return on;
}

template <int HD>
static int launch_decode_t(const uint16_t* q, const uint16_t* kpool, const uint16_t* vpool, int bs,
                           const int32_t* bt, int MB, const int32_t* ctx, int B, int nh, int nkv,
                           uint16_t* out, void* scratch, hipStream_t s, bool tickets_zeroed, int R, int num_blocks, int window) {
  const int G = nh / nkv, Bs = B / R, NS = attn_decode_splits(Bs, nkv);   // Bs sequences of R batch rows each
  // in-launch merge: needs every split's work-group resident on a CU of its own (grid <= CUs) and
  // the ticket counters at zero (the model keeps them so; the per-op entry cannot know)
  int num_cu = 0;
  if (device_num_cu(&num_cu) != MI_OK) return MI_EHIP;
  const bool merge = attn_merge_enabled() && R == 1 && NS > 1 && tickets_zeroed && NS * nkv * B <= num_cu && nkv * B <= kAttnTickets;
  unsigned int* tickets = reinterpret_cast<unsigned int*>(scratch);
  float* ml_part = reinterpret_cast<float*>(tickets + kAttnTickets);
  float* o_part = ml_part + (size_t)B * nh * kAttnMaxSplits * 2;
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)HD);
  constexpr size_t lds8 = attn_decode_lds<HD, 8>(), lds4 = attn_decode_lds<HD, 4>();
  constexpr size_t kMergeLds = 96 * 1024;   // more than half a CU's LDS: one work-group per CU (see the kernel comment)
  if (window > 0) {
    // sliding window: the same split count, partial layout and combine; no in-launch merge, no early K/V request
    MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_kernel<HD, 8, true, false, true>), (int)lds8));
    MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_kernel<HD, 4, false, false, true>), (int)lds4));
    if (NS == 1) {
      hipLaunchKernelGGL((attn_decode_kernel<HD, 8, true, false, true>), dim3(1, nkv, Bs), dim3(512), lds8, s, q, kpool, vpool, bs,
                         bt, MB, ctx, nh, nkv, G, 1, nullptr, nullptr, out, scale_log2e, nullptr, R, 0, window);
    } else {
      hipLaunchKernelGGL((attn_decode_kernel<HD, 4, false, false, true>), dim3(NS, nkv, Bs), dim3(256), lds4, s, q, kpool, vpool,
                         bs, bt, MB, ctx, nh, nkv, G, NS, o_part, ml_part, nullptr, scale_log2e, nullptr, R, 0, window);
      hipLaunchKernelGGL((attn_combine_kernel<HD>), dim3(nh, B), dim3(HD), 0, s, o_part, ml_part, NS, nh, out);
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
  }
  {
    int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_kernel<HD, 8, true>), (int)lds8);
    if (rc == MI_OK) rc = ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_kernel<HD, 4, false>), (int)lds4);
    if (rc == MI_OK) rc = ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_kernel<HD, 4, false, true>), (int)kMergeLds);
    if (rc != MI_OK) return rc;
  }
  if (NS == 1) {
    // Enough (sequence, kv head) pairs to fill the chip: one launch, no partials.  (Measured: a
    // single CU sustains only ~32 GB/s from HBM however many loads its waves keep in flight, so
    // a short grid must split the context over CUs -- the one-launch form at B x nkv = 32 took
    // 16 us per 1k tokens of context against 8 + 5 us for split + combine.)
    hipLaunchKernelGGL((attn_decode_kernel<HD, 8, true>), dim3(1, nkv, Bs), dim3(512), lds8, s, q,
                       kpool, vpool, bs, bt, MB, ctx, nh, nkv, G, 1, nullptr, nullptr, out, scale_log2e, nullptr, R, num_blocks);
  } else if (merge) {
    hipLaunchKernelGGL((attn_decode_kernel<HD, 4, false, true>), dim3(NS, nkv, B), dim3(256), kMergeLds, s, q,
                       kpool, vpool, bs, bt, MB, ctx, nh, nkv, G, NS, o_part, ml_part, out, scale_log2e, tickets);
  } else {
    hipLaunchKernelGGL((attn_decode_kernel<HD, 4, false>), dim3(NS, nkv, Bs), dim3(256), lds4, s, q,
                       kpool, vpool, bs, bt, MB, ctx, nh, nkv, G, NS, o_part, ml_part, nullptr, scale_log2e, nullptr, R, num_blocks);
    hipLaunchKernelGGL((attn_combine_kernel<HD>), dim3(nh, B), dim3(HD), 0, s, o_part, ml_part, NS, nh, out);
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_attn_decode(const uint16_t* q, const uint16_t* kpool, const uint16_t* vpool, int block_size,
                       const int32_t* block_table, int MB, const int32_t* ctx_lens, int B, int nh,
                       int nkv, int hd, uint16_t* out, void* scratch, hipStream_t s, bool tickets_zeroed, int rows_per_seq,
                       int num_blocks, int window) {
  MI_CHECK(hd == 64 || hd == 128, "attention: head_dim must be 64 or 128");
  MI_CHECK(window >= 0, "attention: the sliding window must be >= 0 (0 = none)");
  if ((long)MB * block_size <= window) window = 0;   // no row of this table can hold a key outside the window: the unwindowed launch
  MI_CHECK(rows_per_seq >= 1 && B % rows_per_seq == 0 && (nh / nkv) * rows_per_seq <= 16,
           "attention: rows_per_seq must divide the batch and q heads per kv head x rows_per_seq must be <= 16");
  MI_CHECK(nh % nkv == 0 && nh / nkv <= 16, "attention: q heads per kv head must be 1..16");
  MI_CHECK(block_size % 16 == 0, "attention: block_size must be a multiple of 16");
  if (hd == 128) return launch_decode_t<128>(q, kpool, vpool, block_size, block_table, MB, ctx_lens, B, nh, nkv, out, scratch, s, tickets_zeroed, rows_per_seq, num_blocks, window);
  return launch_decode_t<64>(q, kpool, vpool, block_size, block_table, MB, ctx_lens, B, nh, nkv, out, scratch, s, tickets_zeroed, rows_per_seq, num_blocks, window);
}

// =====================================================================================
// token generation over an FP8 (e4m3) pool
// =====================================================================================
// The same grid, context-split dealing, partial layout and combine as attn_decode_kernel; what differs is how the
// bytes travel.  A K/V row is HD BYTES, so a wave walks 64-token tiles (8 KiB of K + 8 KiB of V at head_dim 128: the
// bytes of a bf16 32-token tile), two in flight: 2 x 16 KiB per wave at long context, as the bf16 kernel has.  A tile
// is four 16-token groups that each look their own block up (block_size 16 / 32 / 48 ...), consumed as two 32-token
// halves through the bf16 kernel's S^T / softmax / P.V step.  All MFMAs are v_mfma_f32_16x16x32_bf16: the codes are
// widened to bf16 in registers (exact), q / P / the output keep their bf16 rounding points, k_scale rides in the
// score scale and v_scale multiplies the wave-merged output once.
//   K: lane (g, c) of a 16-token group loads 16 bytes of token c: dims 64 j + 16 g .. + 15 (j < HD / 64) with ONE
//      global_load_dwordx4.  The 16 codes decode to two A fragments, so k-step 2 j + e of lane g covers dims
//      64 j + 16 g + 8 e .. + 7; the q fragments are loaded once with the same map (a dot product does not care
//      in which order the dimensions are summed as long as both operands agree).
//   V: whole rows (lane-linear 16-byte chunks) parked as BYTES in a wave-private LDS tile, row pitch HD + 16.  Token
//      32 h + 16 u + 4 g + i of the tile is parked at row 32 h + 8 g + 4 u + i, so the 8 k-slots of lane group g in
//      half h -- bound to tokens 4 g + j (j < 4) and 16 + 4 g + j - 4, where the two S^T accumulators hold their
//      scores -- are the 8 CONSECUTIVE rows 32 h + 8 g ..  ds_read_b64_tr_b8 then delivers the A operand whole:
//      within a 16-lane group lane 2 r + p addresses row r, bytes 8 p .. 8 p + 7 of a 16-dim column block, and lane
//      i receives byte i of the 8 rows = V^T[16 dn + i][k-slots 8 g .. 8 g + 7] (ONE transposed read per MFMA; the
//      bf16 kernel needs two).  A half-wave reads 16 consecutive rows: 16 different 4-bank windows at this pitch.
// Masking is by score (P = 0), so EVERY byte the kernel may fetch -- tokens past the context inside a live half, groups
// read from the null block, the clamped early fetch -- must be a finite code: P = 0 times the e4m3 NaN code (0x7F / 0xFF)
// would poison the accumulator.  The write rule saturates and the pool's owner zero-fills it, so the library's own pool
// never holds one; a caller of mi_op_paged_attn_decode_f8 that owns its pool must keep that promise.
typedef __attribute__((ext_vector_type(2))) int i32x2_t;

// SW: attn_decode_kernel's sliding window over 64-token tiles (t_lo = max(0, min ctx_r - W) / 64); a 32-token half that lies
// wholly below every row's window is skipped like one beyond the context.
template <int HD, int NW, bool FINAL, bool SW = false>
__global__ __launch_bounds__(NW * 64) void attn_decode_f8_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kpool, const uint8_t* __restrict__ vpool,
    int bs, const int32_t* __restrict__ block_table, int MB, const int32_t* __restrict__ ctx_lens,
    int nh, int nkv, int G, int NS, float* __restrict__ o_part, float* __restrict__ ml_part,
    uint16_t* __restrict__ out, float score_scale, float v_scale, int R, int num_blocks, int window = 0) {
  constexpr int TT = 64;            // tokens per tile
  constexpr int KPB = HD + 16;      // LDS row pitch (bytes)
  constexpr int CPR = HD / 16;      // 16-byte chunks per row
  constexpr int KJ = HD / 64;       // 16-byte K loads per lane and 16-token group
  constexpr int KS = HD / 32, DN = HD / 16;
  constexpr int NK = 4 * KJ;        // 16-byte K loads per lane per tile
  constexpr int NV = TT * CPR / 64; // 16-byte V loads per lane per tile
  constexpr int VT = TT * KPB;      // bytes of one wave's V tile (>= the 16 x HD fp32 the wave merge parks there)
  static_assert(VT >= 16 * HD * 4, "the wave merge reuses the V tile");
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float* sm_ml = reinterpret_cast<float*>(dsm + (size_t)NW * VT);    // [NW][16][2]

  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z * R;   // b: first batch row of the sequence
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int Gc = G * R;                         // live MFMA columns (see attn_decode_kernel for R > 1)
  const int cr = c / G, ch = c - cr * G;
  int ctx = 0;
  for (int r = 0; r < R; ++r) ctx = max(ctx, ctx_lens[b + r]);
  const int ctx_c = c < Gc ? ctx_lens[b + cr] : 0;
  int key_lo = 0;                               // SW: the first key any row's window holds
  if constexpr (SW) {
    int lo = ctx;
    for (int r = 0; r < R; ++r) lo = min(lo, ctx_lens[b + r]);
    key_lo = max(lo - window, 0);
  }
  const int lo_c = SW ? ctx_c - window : 0;     // SW: the first key of this lane's column
  const int nt = ceil_div(ctx, TT), stride = NS * NW;
  const int t_first = key_lo / TT + split * NW + wave, t_end = nt;
  unsigned char* Vw = dsm + (size_t)wave * VT;

  u32x4_t kA[NK], vA[NV], kB[NK], vB[NV];
  // EARLY (num_blocks > 0, the wave's first tile only): no use of the context length; the table index and the block
  // id are clamped into range, and what was fetched is masked by score or never consumed.  Otherwise a group beyond
  // the context (and possibly beyond the table) reads the null block, a tile beyond the wave's range one line of it.
  auto issue = [&](u32x4_t (&kr)[NK], u32x4_t (&vr)[NV], int tt, bool early) {
    const bool live = early || tt < t_end;
    const int tok0 = live ? tt * TT : 0;
    size_t rowh[4];   // pool row of the first token of each 16-token group
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tok = tok0 + 16 * u;
      int blk;
      bool in;
      if (early) {
        in = true;
        blk = min(max(block_table[(size_t)b * MB + min(tok / bs, MB - 1)], 0), num_blocks - 1);
      } else {
        in = live && tok < ctx;
        blk = in ? block_table[(size_t)b * MB + tok / bs] : 0;
      }
      rowh[u] = in ? ((size_t)blk * nkv + kvh) * bs + (tok % bs) : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t kbase = live ? (rowh[u] + c) * HD + g * 16 : 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j)
        kr[u * KJ + j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(kpool + kbase + (live ? 64 * j : 0)));
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (lane + 64 * i) / CPR, chn = (lane + 64 * i) % CPR;   // row of the tile, 16-byte chunk of the row
      const size_t src = live ? (rowh[row >> 4] + (row & 15)) * HD + chn * 16 : 0;
      vr[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(vpool + src));
    }
  };
  issue(kA, vA, t_first, !SW && num_blocks > 0);

  // q fragment (j, e) of lane (g, c): head column c, dims 64 j + 16 g + 8 e .. + 7
  u32x4_t qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = (c < Gc) ? *reinterpret_cast<const u32x4_t*>(q + ((size_t)(b + cr) * nh + kvh * G + ch) * HD + 64 * (ks >> 1) + 16 * g + 8 * (ks & 1))
                      : u32x4_t{0, 0, 0, 0};
  f32x4_t acc[DN];
#pragma unroll
  for (int dn = 0; dn < DN; ++dn) acc[dn] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float mrow = -INFINITY, lrow = 0.f;   // head c: running max (same on its 4 lanes), this lane's share of the sum
  const int tr_off = (8 * g + (c >> 1)) * KPB + 8 * (c & 1);   // transposed read: row 8 g + c / 2, byte half c % 2

  auto update = [&](const u32x4_t (&kr)[NK], const u32x4_t (&vr)[NV], int tt) {
    // park V (the previous tile's transposed reads are complete: their values fed MFMAs already)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int row = (lane + 64 * i) / CPR, chn = (lane + 64 * i) % CPR;
      const int prow = (row & 32) | (((row >> 2) & 3) << 3) | (((row >> 4) & 1) << 2) | (row & 3);
      *reinterpret_cast<u32x4_t*>(Vw + prow * KPB + chn * 16) = vr[i];
    }
    asm volatile("" ::: "memory");   // LDS ops of one wave execute in order; keep the compiler from reordering them
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int tok0 = tt * TT + 32 * h;
      if (tok0 >= ctx) break;         // wave-uniform: the whole half lies beyond the context
      if constexpr (SW) { if (tok0 + 32 <= key_lo) continue; }   // ... or below every row's window
      f32x4_t st[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        st[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          const u32x4_t kw = kr[(2 * h + u) * KJ + j];
          st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(decode8<MI_W_F8E4M3>(kw[0], kw[1]), __builtin_bit_cast(bf16x8_t, qf[2 * j]), st[u], 0, 0, 0);
          st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(decode8<MI_W_F8E4M3>(kw[2], kw[3]), __builtin_bit_cast(bf16x8_t, qf[2 * j + 1]), st[u], 0, 0, 0);
        }
      }
      i32x2_t vt[DN];
#pragma unroll
      for (int dn = 0; dn < DN; ++dn)
        vt[dn] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((i32x2_t __attribute__((address_space(3)))*)(Vw + 32 * h * KPB + tr_off + 16 * dn));
      float pv[8];
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float sv = st[u][i] * score_scale;
          if (tok0 + 16 * u + 4 * g + i >= ctx_c) sv = -INFINITY;
          if constexpr (SW) { if (tok0 + 16 * u + 4 * g + i < lo_c) sv = -INFINITY; }
          pv[4 * u + i] = sv;
          mx = fmaxf(mx, sv);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));       // -inf where the column has no live token in this half (sexp2 conventions)
      const float mn = fmaxf(mrow, mx);
      const float alpha = sexp2(mrow, mn);
      float ps = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        pv[k] = sexp2(pv[k], mn);
        ps += pv[k];
      }
      const bool moved = mn != mrow;
      mrow = mn;
      lrow = lrow * alpha + ps;
      union { uint32_t w[4]; bf16x8_t v; } pk;
#pragma unroll
      for (int k = 0; k < 4; ++k) pk.w[k] = pack_bf16x2(pv[2 * k], pv[2 * k + 1]);
      if (__any(moved)) {
#pragma unroll
        for (int dn = 0; dn < DN; ++dn) {
          acc[dn][0] *= alpha; acc[dn][1] *= alpha; acc[dn][2] *= alpha; acc[dn][3] *= alpha;
        }
      }
#pragma unroll
      for (int dn = 0; dn < DN; ++dn)
        acc[dn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(decode8<MI_W_F8E4M3>((uint32_t)vt[dn][0], (uint32_t)vt[dn][1]), pk.v, acc[dn], 0, 0, 0);
    }
  };

  for (int tt = t_first; tt < t_end; tt += 2 * stride) {
    issue(kB, vB, tt + stride, false);
    update(kA, vA, tt);
    issue(kA, vA, tt + 2 * stride, false);
    if (tt + stride < t_end) update(kB, vB, tt + stride);
  }

  // ---- merge the waves: O^T / m / l of wave w go to its own (now idle) LDS tile --------------
  lrow += __shfl_xor(lrow, 16);
  lrow += __shfl_xor(lrow, 32);
  asm volatile("" ::: "memory");
  float* so = reinterpret_cast<float*>(Vw);            // [16 heads][HD] f32
#pragma unroll
  for (int dn = 0; dn < DN; ++dn) *reinterpret_cast<f32x4_t*>(&so[c * HD + 16 * dn + 4 * g]) = acc[dn];
  if (g == 0) {
    sm_ml[(wave * 16 + c) * 2] = mrow;
    sm_ml[(wave * 16 + c) * 2 + 1] = lrow;
  }
  __syncthreads();
  for (int idx = tid; idx < Gc * HD; idx += NW * 64) {
    const int h = idx / HD, d = idx % HD;       // h: MFMA column
    const int hr = h / G, hh = h - hr * G;      // -> (row of the sequence, head)
    float M = sm_ml[h * 2];
#pragma unroll
    for (int w = 1; w < NW; ++w) M = fmaxf(M, sm_ml[(w * 16 + h) * 2]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {  // wave order: deterministic
      const float f = sexp2(sm_ml[(w * 16 + h) * 2], M);
      o += f * reinterpret_cast<const float*>(dsm + (size_t)w * VT)[h * HD + d];
      L += f * sm_ml[(w * 16 + h) * 2 + 1];
    }
    if constexpr (FINAL) {
      out[((size_t)(b + hr) * nh + kvh * G + hh) * HD + d] = f32_to_bf16(L > 0.f ? o / L * v_scale : 0.f);   // empty context -> zeros
    } else {
      const size_t row = ((size_t)(b + hr) * nh + kvh * G + hh) * kAttnMaxSplits + split;
      o_part[row * HD + d] = o * v_scale;
      if (d == 0) {
        ml_part[row * 2] = M;
        ml_part[row * 2 + 1] = L;
      }
    }
  }
}
template <int HD, int NW>
constexpr size_t attn_decode_f8_lds() { return (size_t)NW * 64 * (HD + 16) + (size_t)NW * 16 * 2 * sizeof(float); }

template <int HD>
static int launch_decode_f8_t(const uint16_t* q, const uint8_t* kpool, const uint8_t* vpool, int bs, const int32_t* bt,
                              int MB, const int32_t* ctx, int B, int nh, int nkv, float k_scale, float v_scale,
                              uint16_t* out, void* scratch, hipStream_t s, int R, int num_blocks, int window) {
  const int G = nh / nkv, Bs = B / R, NS = attn_decode_splits(Bs, nkv);   // Bs sequences of R batch rows each
  float* ml_part = reinterpret_cast<float*>(reinterpret_cast<unsigned int*>(scratch) + kAttnTickets);
  float* o_part = ml_part + (size_t)B * nh * kAttnMaxSplits * 2;
  const float score_scale = 1.4426950408889634f / sqrtf((float)HD) * k_scale;
  constexpr size_t lds8 = attn_decode_f8_lds<HD, 8>(), lds4 = attn_decode_f8_lds<HD, 4>();
  MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_f8_kernel<HD, 8, true>), (int)lds8));
  MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_f8_kernel<HD, 4, false>), (int)lds4));
  if (window > 0) {
    MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_f8_kernel<HD, 8, true, true>), (int)lds8));
    MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_decode_f8_kernel<HD, 4, false, true>), (int)lds4));
    if (NS == 1) {
      hipLaunchKernelGGL((attn_decode_f8_kernel<HD, 8, true, true>), dim3(1, nkv, Bs), dim3(512), lds8, s, q, kpool, vpool, bs, bt,
                         MB, ctx, nh, nkv, G, 1, nullptr, nullptr, out, score_scale, v_scale, R, 0, window);
    } else {
      hipLaunchKernelGGL((attn_decode_f8_kernel<HD, 4, false, true>), dim3(NS, nkv, Bs), dim3(256), lds4, s, q, kpool, vpool, bs, bt,
                         MB, ctx, nh, nkv, G, NS, o_part, ml_part, nullptr, score_scale, v_scale, R, 0, window);
      hipLaunchKernelGGL((attn_combine_kernel<HD>), dim3(nh, B), dim3(HD), 0, s, o_part, ml_part, NS, nh, out);
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
  }
  if (NS == 1) {
    hipLaunchKernelGGL((attn_decode_f8_kernel<HD, 8, true>), dim3(1, nkv, Bs), dim3(512), lds8, s, q, kpool, vpool, bs, bt,
                       MB, ctx, nh, nkv, G, 1, nullptr, nullptr, out, score_scale, v_scale, R, num_blocks);
  } else {
    hipLaunchKernelGGL((attn_decode_f8_kernel<HD, 4, false>), dim3(NS, nkv, Bs), dim3(256), lds4, s, q, kpool, vpool, bs, bt,
                       MB, ctx, nh, nkv, G, NS, o_part, ml_part, nullptr, score_scale, v_scale, R, num_blocks);
    hipLaunchKernelGGL((attn_combine_kernel<HD>), dim3(nh, B), dim3(HD), 0, s, o_part, ml_part, NS, nh, out);
  }
  MI_HIP(hipGetLastError());
  return MI_OK;
}

int launch_attn_decode_f8(const uint16_t* q, const uint8_t* kpool, const uint8_t* vpool, int block_size,
                          const int32_t* block_table, int MB, const int32_t* ctx_lens, int B, int nh, int nkv, int hd,
                          float k_scale, float v_scale, uint16_t* out, void* scratch, hipStream_t s, int rows_per_seq,
                          int num_blocks, int window) {
  MI_CHECK(hd == 64 || hd == 128, "attention: head_dim must be 64 or 128");
  MI_CHECK(window >= 0, "attention: the sliding window must be >= 0 (0 = none)");
  if ((long)MB * block_size <= window) window = 0;   // no row of this table can hold a key outside the window: the unwindowed launch
  MI_CHECK(rows_per_seq >= 1 && B % rows_per_seq == 0 && (nh / nkv) * rows_per_seq <= 16,
           "attention: rows_per_seq must divide the batch and q heads per kv head x rows_per_seq must be <= 16");
  MI_CHECK(nh % nkv == 0 && nh / nkv <= 16, "attention: q heads per kv head must be 1..16");
  MI_CHECK(block_size % 16 == 0, "attention: block_size must be a multiple of 16");
  MI_CHECK(MB >= 1 && k_scale > 0.f && v_scale > 0.f, "attention: the block table width and the FP8 KV scales must be positive");
  if (hd == 128) return launch_decode_f8_t<128>(q, kpool, vpool, block_size, block_table, MB, ctx_lens, B, nh, nkv, k_scale, v_scale, out, scratch, s, rows_per_seq, num_blocks, window);
  return launch_decode_f8_t<64>(q, kpool, vpool, block_size, block_table, MB, ctx_lens, B, nh, nkv, k_scale, v_scale, out, scratch, s, rows_per_seq, num_blocks, window);
}

// =====================================================================================
// context encoding: 32x32x16 MFMAs, K/V tiles by LDS-DMA, two waves per SIMD
// =====================================================================================
// What the counters of the first-generation kernel asked for (17 % MFMA-busy at one wave per
// SIMD, 408 registers, 144 accumulator moves and a ds_write staging pass per 64-key tile):
//   * a wave owns ONE 32-query block of one q head: S^T[key][q] = K . Q^T on v_mfma_f32_32x32x16_bf16
//     puts a query on a lane (its 32 scores of a 64-key tile in 32 registers of lanes l and l + 32), so
//     the row maximum / sum is 31 VALU ops and ONE v_permlane32_swap, and the exponentiated
//     accumulators, packed pairwise to bf16, ARE the B operand of O^T[d][q] += V^T . P^T (k-slot j of
//     lane half h <-> key 16 s + 8 (j >> 2) + 4 h + (j & 3): the transposed V reads are bound to that order);
//   * K and V tiles (64 keys) arrive by LDS-DMA (global_load_lds, 1 KiB per wave-instruction) into a
//     ring of three 32 KiB stages: no staging registers, no ds_write, two tiles in flight while one is
//     multiplied, retired by a counted vmcnt in front of ONE raw barrier per tile.  The paged pool is
//     addressed per piece (4 keys x 256 B at head_dim 128): the block id is a scalar load, the per-lane
//     part of the source address is constant for the whole kernel;
//   * the LDS image is rows of head_dim bf16 whose 16-byte chunks are XOR-swizzled by the key (applied
//     to the per-lane SOURCE address of the DMA and to the reads): conflict-free for the ds_read_b128
//     row reads of K (16 lanes = 16 keys = 16 different slots) and for the ds_read_b64_tr_b16
//     transposed reads of V (a half-wave's 4 keys land on 4 different 64-byte windows);
//   * ~170 registers: two waves per SIMD.  A work-group is NW waves = QB query blocks x Gp q heads of
//     one kv group, all sharing the K/V ring.  Causal work grows with the block index, so the QB blocks
//     of a work-group are complementary pairs (j, nblk - 1 - j): every SIMD of the chip gets the same
//     number of key tiles, and the light block's waves keep issuing DMAs for the heavy one's tail.
// Softmax: the running maximum used in the exponent is only moved when the tile's maximum exceeds it
// by more than kDeferLog2 (deferred rescale): p <= 2^kDeferLog2 instead of <= 1, O and l carry the
// same factor, the quotient O / l is unchanged up to rounding; the 64-register rescale of O^T becomes rare.
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
constexpr float kDeferLog2 = 6.f;

// {v of this lane, v of lane ^ 32} in some order (max / sum do not care): one v_permlane32_swap.  The elements of the
// builtin's result are copied out before the bit cast: hipcc 7.2 reads element 0 for __builtin_bit_cast(float, r[1])
// (hipcc notes) -- which made a row's sum 2 x (its lower half's sum).
__device__ __forceinline__ f32x2_t swap32_pair(float v) {
  const unsigned a = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(a, a, false, false);
  const unsigned r0 = r[0], r1 = r[1];
  return f32x2_t{__builtin_bit_cast(float, r0), __builtin_bit_cast(float, r1)};
}

template <int HD>
__device__ __forceinline__ int kv_swz(int key) {   // XOR key of the 16-byte chunk index of a K/V row in LDS
  if constexpr (HD == 128) return ((key & 3) << 2) | ((key >> 2) & 3);          // 256-byte rows, 16 chunks
  else return (((key >> 1) & 1) << 2) | ((key >> 2) & 3);                        // 128-byte rows,  8 chunks
}

// The sizes the two kernels and their launchers agree on.
template <int HD>
struct PrefillTile {
  static constexpr int TK = 64;                // keys per tile
  static constexpr int ROWB = HD * 2;          // bytes per K/V row of the bf16 image
  static constexpr int KIMG = TK * ROWB;       // bf16 image of a K (or V) tile: 16 / 8 KiB
  static constexpr int ISTAGE = 2 * KIMG;      // K image, V image
  static constexpr int CSTAGE = 2 * TK * HD;   // the same tile as FP8 codes: K part, V part
  static constexpr int NSTAGE = 3;             // stages of the DMA ring (of images in the bf16 kernel, of codes in the f8 kernel)
};
template <int HD>
constexpr int attn_prefill_lds() { return PrefillTile<HD>::NSTAGE * PrefillTile<HD>::ISTAGE; }
template <int HD>   // the code ring and a double-buffered image
constexpr int attn_prefill_f8_lds() { return PrefillTile<HD>::NSTAGE * PrefillTile<HD>::CSTAGE + 2 * PrefillTile<HD>::ISTAGE; }

//
// SW (sliding window W >= 1, launched only when q_pos0 + T > W): query p attends the keys p - W < k <= p, so the work of a
// 32-query block is a BAND of about (W + 95) / 64 key tiles whatever its index, and the bands of a heavy and a light block
// do not overlap: a pair sharing a ring would stream tiles only one of them wants.  A work-group therefore owns the QB =
// NW / Gp ADJACENT blocks blockIdx.x QB .. + QB - 1 (same head slots), one pass, and its ring walks the union of their
// bands: tiles t_lo_wg = max(0, q_pos0 + q0_first - W + 1) / 64 .. the last tile of its last block.  Every wave issues
// its share of every tile's DMA pieces and passes every barrier, but runs MFMAs and softmax only on the tiles of its own
// band.  The lower-edge mask (key < qpos - W + 1) is applied on tiles that straddle the edge of one of the wave's queries,
// the causal mask on diagonal tiles as before.  A row can meet a tile with no live key before its first live one (its edge
// lies further right than its block's first): its running maximum stays -inf and the exponent takes 0 in its place, so
// p = exp2(-inf) = 0 and neither l nor O moves.
template <int HD, int NW, bool SW = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_prefill2_kernel(
    const uint16_t* __restrict__ q, int T, int q_pos0, const uint16_t* __restrict__ kpool,
    const uint16_t* __restrict__ vpool, int bs, int bs_shift, const int32_t* __restrict__ block_table, int nh, int nkv,
    int G, int Gp, int nblk, uint16_t* __restrict__ out, float scale_log2e, int window = 0) {
  using P = PrefillTile<HD>;
  constexpr int TK = P::TK, ROWB = P::ROWB, KBYTES = P::KIMG, STAGE = P::ISTAGE, NSTAGE = P::NSTAGE;
  constexpr int CPR = HD / 8;                  // 16-byte chunks per row
  constexpr int KPP = 1024 / ROWB;             // keys per 1 KiB DMA piece (4 / 8)
  constexpr int NP = TK / KPP;                 // pieces per K (or V) tile (16 / 8)
  constexpr int PPW = NP / NW > 0 ? NP / NW : 1;   // K pieces per wave and tile (V the same)
  static_assert(NP % NW == 0, "pieces must divide over the waves");
  constexpr int CNT = 2 * PPW;                 // DMA instructions per wave and tile
  constexpr int KSTEPS = HD / 16, DB = HD / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kvh = blockIdx.y;
  const int QB = NW / Gp;
  const int hl = wave % Gp, slot = wave / Gp;
  const int head = kvh * G + min(hl, G - 1);
  const bool head_ok = hl < G;
  const int kv_len = q_pos0 + T;
  const int last_piece_key = ((kv_len - 1) / KPP) * KPP;
  const int qq = lane & 31, h = lane >> 5;
  const int npair = (nblk + 1) >> 1;

  // ---- per-lane constants of the LDS image -------------------------------------------------------
  // DMA: lane i of a piece fills slot (i % CPR) of key (i / CPR) of the piece: it fetches the chunk the swizzle puts there
  const int kip = lane / CPR, dslot = lane % CPR;
  int dma_sw;
  if constexpr (HD == 128) dma_sw = (kip << 2) | (wave & 3);                 // kv_swz(4 piece + kip), piece = wave (mod 4)
  else dma_sw = (((kip >> 1) & 1) << 2) | ((2 * (wave & 1) + (kip >> 2)) & 3);   // kv_swz(8 piece + kip), piece = wave (mod 2)
  const int dma_lane_off = kip * HD + ((dslot ^ dma_sw) * 8);                // elements, relative to the piece's first row
  // K row reads (A operand of S^T): key qq of a 32-key block, chunk 2 ks + h
  int kaddr[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) kaddr[ks] = qq * ROWB + (((2 * ks + h) ^ kv_swz<HD>(qq)) * 16);
  // V transposed reads (A operand of O^T): group gi = lane >> 4 covers dims 16 (gi & 1) .. + 15 of a 32-dim block for lane half
  // h = gi >> 1; lane 4 qr + pc of the group addresses key row (4 h + qr [+ 8]) at dims 4 pc .. 4 pc + 3
  const int gi = lane >> 4, qr = (lane & 15) >> 2, pc = lane & 3;
  int vaddr[DB][2];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = 4 * h + qr + 8 * u;                                     // (+ 32 b + 16 s: no effect on the swizzle key)
      const int chunk = 4 * db + 2 * (gi & 1) + (pc >> 1);
      vaddr[db][u] = key * ROWB + ((chunk ^ kv_swz<HD>(key)) * 16) + 8 * (pc & 1);
    }

  const int passes = (!SW && QB == 1) ? 2 : 1;
  for (int pass = 0; pass < passes; ++pass) {
    // ---- which query block this wave owns --------------------------------------------------------
    int blk_q, pair;
    bool blk_ok;
    if constexpr (SW) {                  // adjacent blocks
      pair = 0;
      blk_q = (int)blockIdx.x * QB + slot;
      blk_ok = blk_q < nblk;
    } else if (QB == 1) {                // one block at a time: the heavy one of pair blockIdx.x, then the light one
      pair = blockIdx.x;
      blk_q = pass == 0 ? nblk - 1 - pair : pair;
      blk_ok = pair < npair && !(pass == 1 && pair == nblk - 1 - pair);
    } else {
      pair = (int)blockIdx.x * (QB >> 1) + (slot >> 1);
      blk_q = (slot & 1) ? nblk - 1 - pair : pair;
      blk_ok = pair < npair && !((slot & 1) && pair == nblk - 1 - pair);
    }
    const int q0 = blk_q * 32;
    const bool active = blk_ok && head_ok;
    // tiles: this wave's, and the work-group's (the heaviest block any of its waves owns)
    const int p_first = q_pos0 + min(q0, T - 1), p_last = q_pos0 + min(q0 + 31, T - 1);
    const int nt_wave = active ? p_last / TK + 1 : 0;
    int wg_pair0 = QB == 1 ? (int)blockIdx.x : (int)blockIdx.x * (QB >> 1);
    int wg_blk = QB == 1 ? (pass == 0 ? nblk - 1 - wg_pair0 : wg_pair0) : nblk - 1 - wg_pair0;   // heaviest block of the work-group
    if constexpr (SW) wg_blk = (int)blockIdx.x * QB + QB - 1;                                    // SW: its last block
    wg_blk = max(min(wg_blk, nblk - 1), 0);
    const int nt = (q_pos0 + min(wg_blk * 32 + 31, T - 1)) / TK + 1;
    // SW: first tile of the work-group's ring and of this wave's band; first key of this lane's query (below)
    const int t0 = SW ? max(q_pos0 + (int)blockIdx.x * QB * 32 - window + 1, 0) / TK : 0;
    const int t_lo_wave = SW ? max(p_first - window + 1, 0) / TK : 0;

    // ---- Q fragments (B operand of S^T): Q[q0 + qq][16 ks + 8 h ..] ---------------------------------
    const int qi = min(q0 + qq, T - 1);
    const int qpos = q_pos0 + qi;
    const int klo = SW ? qpos - window + 1 : 0;
    u32x4_t qf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      qf[ks] = active ? *reinterpret_cast<const u32x4_t*>(q + ((size_t)qi * nh + head) * HD + ks * 16 + h * 8) : u32x4_t{0, 0, 0, 0};

    f32x16_t o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m_used = -INFINITY, lsum = 0.f;

    // Block ids are fetched (scalar loads) one tile ahead of the DMAs that use them: the round trip to the scalar cache / L2
    // runs under a tile's arithmetic instead of in front of the global_load_lds it feeds.
    int pf_blk[PPW], pf_off[PPW];
    auto fetch_ids = [&](int t) {
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int k0 = min(t * TK + (wave + NW * i) * KPP, last_piece_key);   // rows past the context: the last piece again (masked by position)
        int bi;
        if (bs_shift >= 0) { bi = k0 >> bs_shift; pf_off[i] = k0 & (bs - 1); }
        else { bi = k0 / bs; pf_off[i] = k0 - bi * bs; }
        pf_blk[i] = block_table[bi];
      }
    };
    auto issue = [&](int st) {                  // the tile whose ids fetch_ids loaded last
      unsigned char* base = smem + st * STAGE;
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int piece = wave + NW * i;
        const size_t row = ((size_t)pf_blk[i] * nkv + kvh) * bs + pf_off[i];
        glds16(kpool + row * HD + dma_lane_off, base + piece * 1024);
        glds16(vpool + row * HD + dma_lane_off, base + KBYTES + piece * 1024);
      }
    };

    int st_issue = 0, st_read = 0;
    fetch_ids(t0);
    issue(0);
    if (nt > t0 + 1) { fetch_ids(t0 + 1); issue(1); }
    fetch_ids(t0 + 2);
    st_issue = 2;
    // hipcc waits for a plain load at its first use -- inside the tile loop, as vmcnt(0) on every iteration, which would drain
    // the two tiles in flight each time.  Taking the Q fragments through an empty asm here puts that wait in front of the loop.
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) asm volatile("" : "+v"(qf[ks]));
    for (int t = t0; t < nt; ++t) {
      if (t + 1 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CNT) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();            // every wave's pieces of tile t are in; everyone is done reading tile t - 1
      if (t + 2 < nt) {
        issue(st_issue);
        st_issue = st_issue == NSTAGE - 1 ? 0 : st_issue + 1;
        fetch_ids(t + 3);
      }
      const unsigned char* Kst = smem + st_read * STAGE;
      const unsigned char* Vst = Kst + KBYTES;
      st_read = st_read == NSTAGE - 1 ? 0 : st_read + 1;
      if (t >= nt_wave) continue;                // wave-uniform: the tile lies in this block's future (or the slot is idle)
      if constexpr (SW) { if (t < t_lo_wave) continue; }   // ... or wholly below the window of its first query

      // ---- S^T = K . Q^T : two 32-key blocks.  The K fragments of a block are requested one block ahead of the MFMAs
      // that take them (8 reads in flight; hipcc left to itself issues read -> wait -> MFMA one at a time) ----
      f32x16_t sc[2];
      {
        bf16x8_t kf[KSTEPS];
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) kf[ks] = *reinterpret_cast<const bf16x8_t*>(Kst + kaddr[ks]);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[b][r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KSTEPS; ++ks) {
            sc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], __builtin_bit_cast(bf16x8_t, qf[ks]), sc[b], 0, 0, 0);
            if (b == 0) kf[ks] = *reinterpret_cast<const bf16x8_t*>(Kst + 32 * ROWB + kaddr[ks]);
          }
        }
        __builtin_amdgcn_sched_group_barrier(0x100, KSTEPS, 0);
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
      }
      // ---- online softmax: this lane holds 32 scores of query qq (keys (r & 3) + 8 (r >> 2) + 4 h of each block) ----
      const bool need_mask = t * TK + TK - 1 > p_first;
      if (need_mask) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (t * TK + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h > qpos) sc[b][r] = -INFINITY;
      }
      if constexpr (SW) {
        if (t * TK < p_last - window + 1) {      // the tile straddles the lower edge of one of the wave's queries
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (t * TK + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h < klo) sc[b][r] = -INFINITY;
        }
      }
      float mx = sc[0][0];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[b][r]);
      {
        const f32x2_t sw = swap32_pair(mx);
        mx = fmaxf(sw[0], sw[1]);
      }
      const float ms = mx * scale_log2e;         // key 0 is visible to every query: finite from the first tile on (SW: -inf until the row's first live tile)
      const bool moved = ms > m_used + kDeferLog2;
      if (__any(moved)) {
        const float mn = moved ? ms : m_used;
        const float alpha = moved ? fexp2(m_used - mn) : 1.f;   // exp2(-inf) = 0 on the first tile
        m_used = mn;
        lsum *= alpha;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      }
      // ---- p = exp2(s - m), packed to bf16 = the B operands of O^T += V^T . P^T.  The transposed V fragments of the first
      // kVAhead MFMAs are requested in front of the exponentials (no dependence), the rest kVAhead MFMAs ahead of their use ----
      // The transposed reads are inline asm: behind the builtin hipcc assumes the read may alias the LDS-DMAs in flight and
      // drains them (s_waitcnt vmcnt(0) per tile).  Their completion is counted by hand: LDS reads return in order, and between
      // the first V read of a tile and its last MFMA the wave issues no other LDS or scalar-memory instruction.
      constexpr int NPV = 4 * DB;               // MFMAs: (b, s2) outer, d-block inner
      constexpr int kVAhead = 4;
      s16x4_t vlo[NPV], vhi[NPV];
      unsigned vbase[DB][2];
      const unsigned vst_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)Vst;
#pragma unroll
      for (int db = 0; db < DB; ++db) { vbase[db][0] = vst_lds + vaddr[db][0]; vbase[db][1] = vst_lds + vaddr[db][1]; }
#define MI_VREAD(i_)                                                                                                         \
      do {                                                                                                                   \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vlo[i_]) : "v"(vbase[(i_) % DB][0]), "n"(16 * ((i_) / DB) * ROWB)); \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vhi[i_]) : "v"(vbase[(i_) % DB][1]), "n"(16 * ((i_) / DB) * ROWB)); \
      } while (0)
      MI_VREAD(0); MI_VREAD(1); MI_VREAD(2); MI_VREAD(3);
      static_assert(kVAhead == 4, "the prefetch above is written out for 4");
      bf16x8_t pb[4];
      // SW: a row with no live key so far has m_used = -inf and only masked scores: 0 in its place keeps -inf - m from being NaN
      const float m_exp = (SW && m_used == -INFINITY) ? 0.f : m_used;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float pv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          pv[r] = fexp2(fmaf(sc[b][r], scale_log2e, -m_exp));   // masked: exp2(-inf) = 0
          lsum += pv[r];
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          union { uint32_t w[4]; bf16x8_t v; } pk;
#pragma unroll
          for (int k = 0; k < 4; ++k) pk.w[k] = pack_bf16x2(pv[8 * s2 + 2 * k], pv[8 * s2 + 2 * k + 1]);
          pb[2 * b + s2] = pk.v;
        }
      }
      // ---- O^T += V^T . P^T --------------------------------------------------------------------------
      // before MFMA i: reads issued = 2 min(i + 1 + kVAhead - 1, NPV) ... all but the ones behind fragment i may be outstanding
#define MI_PV(i_)                                                                                                            \
      do {                                                                                                                   \
        constexpr int issued = 2 * ((i_) + kVAhead < NPV ? (i_) + kVAhead : NPV);                                            \
        asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(vlo[i_]), "+v"(vhi[i_]) : "n"(issued - 2 * ((i_) + 1)));               \
        const s16x4_t lo = vlo[i_], hi = vhi[i_];                                                                            \
        const bf16x8_t a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                                         \
        o[(i_) % DB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb[(i_) / DB], o[(i_) % DB], 0, 0, 0);                     \
        if constexpr ((i_) + kVAhead < NPV) MI_VREAD((i_) + kVAhead);                                                        \
      } while (0)
      MI_PV(0); MI_PV(1); MI_PV(2); MI_PV(3); MI_PV(4); MI_PV(5); MI_PV(6); MI_PV(7);
      if constexpr (NPV == 16) { MI_PV(8); MI_PV(9); MI_PV(10); MI_PV(11); MI_PV(12); MI_PV(13); MI_PV(14); MI_PV(15); }
#undef MI_PV
#undef MI_VREAD
    }
    // ---- epilogue: O^T[d][q] / l -> out[q][head][d]; lanes l and l + 32 hold neighbouring 4-dim groups of one query:
    // one v_permlane32_swap per pair of groups makes 16-byte stores of them
    {
      const f32x2_t sw = swap32_pair(lsum);
      lsum = sw[0] + sw[1];
    }
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    const bool st_ok = active && q0 + qq < T;
    uint16_t* orow = out + ((size_t)(q0 + qq) * nh + head) * HD;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int k2 = 0; k2 < 4; k2 += 2) {      // dim groups k2, k2 + 1: dims 32 db + 8 k + 4 h + (0..3)
        uint32_t a0 = pack_bf16x2(o[db][4 * k2 + 0] * inv, o[db][4 * k2 + 1] * inv);
        uint32_t a1 = pack_bf16x2(o[db][4 * k2 + 2] * inv, o[db][4 * k2 + 3] * inv);
        uint32_t b0 = pack_bf16x2(o[db][4 * k2 + 4] * inv, o[db][4 * k2 + 5] * inv);
        uint32_t b1 = pack_bf16x2(o[db][4 * k2 + 6] * inv, o[db][4 * k2 + 7] * inv);
        const auto x = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto y = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        // lower half: [own group k2 | upper's group k2] = dims 8 k2 .. 8 k2 + 7; upper half: [lower's k2 + 1 | own k2 + 1]
        const u32x4_t v = {x[0], y[0], x[1], y[1]};
        if (st_ok) *reinterpret_cast<u32x4_t*>(orow + 32 * db + 8 * (k2 + h)) = v;
      }
    __syncthreads();   // the ring is reused by the next pass
  }
}

// =====================================================================================
// context encoding over an FP8 (e4m3) pool
// =====================================================================================
// attn_prefill2_kernel's work split, MFMA maps, deferred-rescale softmax and epilogue (see there) over the byte pool;
// what differs is how K and V reach the bf16 tile image the MFMAs read.  Codes are widened ONCE per work-group, in LDS:
//   * a K/V row is HD BYTES, a 1 KiB LDS-DMA piece is 1024 / HD keys (8 / 16) of one block and one kv head: contiguous
//     in the pool, so lane i fetches bytes 16 i .. 16 i + 15 of the piece and the DMA needs no swizzled source.  A 64-key
//     tile is NP K pieces + NP V pieces (8 + 8 / 4 + 4); piece p = wave + NW i goes to wave `wave` (head_dim 128: K piece
//     w and V piece w; head_dim 64: waves 0-3 a K piece, waves 4-7 a V piece).  Pieces land in a CODE RING of three
//     stages (K part, V part: 2 x 64 x HD bytes each);
//   * every wave widens the pieces it fetched itself: its own counted vmcnt (no barrier: the code ring is wave-private,
//     a lane even reads back exactly the 16 bytes it fetched), one ds_read_b128, 8 v_cvt_scalef32_pk_bf16_fp8 (exact),
//     two ds_write_b128 into the bf16 TILE IMAGE: rows of HD bf16 with kv_swz<HD> chunks, i.e. what attn_prefill2_kernel's
//     DMA would have left there.  Lanes of neighbouring keys write their two chunks in opposite order, so a group of 16
//     lanes covers 16 different 16-byte slots;
//   * the image is double-buffered.  Iteration t requests tile t + 3, multiplies tile t from image[t & 1], widens tile
//     t + 1 into image[(t + 1) & 1] (under the tail of its own MFMAs), drains its LDS writes and passes ONE raw barrier: image[(t + 1) & 1] is complete for iteration t + 1
//     and nobody still reads image[t & 1] when iteration t + 1 overwrites it with tile t + 2.
// LDS: 3 x 16 KiB + 2 x 32 KiB = 112 KiB at head_dim 128 (56 KiB at 64): one work-group per CU, as the bf16 kernel.
// Numerics: the image holds float(code) exactly, every MFMA is bf16, k_scale rides in the score scale,
// v_scale multiplies the normalised output once; q, P and the output are rounded where attn_prefill2_kernel rounds them.
// The widening's LDS instructions are inline asm (hipcc would drain the DMAs in flight in front of a read that may alias
// them) and sit at the end of the iteration; the window of hand-counted lgkmcnt between the first transposed V read and
// the last P.V MFMA is fenced: s_waitcnt lgkmcnt(0) + sched_barrier(0) in front, sched_barrier(0) behind.
// Masking is by score (P = 0): as for attn_decode_f8_kernel, no byte of a block the table names may be the e4m3 NaN code.
template <int HD, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_prefill_f8_kernel(
    const uint16_t* __restrict__ q, int T, int q_pos0, const uint8_t* __restrict__ kpool,
    const uint8_t* __restrict__ vpool, int bs, int bs_shift, const int32_t* __restrict__ block_table, int nh, int nkv,
    int G, int Gp, int nblk, uint16_t* __restrict__ out, float score_scale, float v_scale) {
  using P = PrefillTile<HD>;
  constexpr int TK = P::TK, ROWB = P::ROWB, KIMG = P::KIMG, ISTAGE = P::ISTAGE, CSTAGE = P::CSTAGE, NSTAGE = P::NSTAGE;
  constexpr int KPP = 1024 / HD;               // keys per 1 KiB piece of codes (8 / 16)
  constexpr int NP = TK / KPP;                 // pieces per K (or V) tile (8 / 4)
  constexpr int CPC = HD / 16;                 // 16-byte code chunks per row
  constexpr int PW = 2 * NP / NW;              // pieces per wave and tile (2 / 1) = DMA instructions per wave and tile
  static_assert(2 * NP % NW == 0 && PW >= 1, "the K and V pieces of a tile must divide over the waves");
  constexpr int KSTEPS = HD / 16, DB = HD / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const img = smem + NSTAGE * CSTAGE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kvh = blockIdx.y;
  const int QB = NW / Gp;
  const int hl = wave % Gp, slot = wave / Gp;
  const int head = kvh * G + min(hl, G - 1);
  const bool head_ok = hl < G;
  const int kv_len = q_pos0 + T;
  const int last_piece_key = ((kv_len - 1) / KPP) * KPP;
  const int qq = lane & 31, h = lane >> 5;
  const int npair = (nblk + 1) >> 1;

  // ---- per-lane constants ------------------------------------------------------------------------
  // widening: lane i of piece p holds codes 16 cc .. 16 cc + 15 (cc = i % CPC) of key KPP (p % NP) + i / CPC of the K
  // (p < NP) or V tile = chunks 2 cc, 2 cc + 1 of that image row; `flip` lanes write the odd chunk first
  const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int cc = lane % CPC;
  unsigned waddr[PW][2], caddr[PW];            // LDS byte addresses: image (relative to its buffer), code ring (to its stage)
  bool flip;
  {
    const int kip = lane / CPC;
    flip = HD == 128 ? (kip & 1) : ((kip >> 1) & 1);
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int p = wave + NW * i, key = KPP * (p % NP) + kip;
      const unsigned row = smem_lds + NSTAGE * CSTAGE + (p >= NP ? KIMG : 0) + key * ROWB;
      waddr[i][0] = row + (((2 * cc + (flip ? 1 : 0)) ^ kv_swz<HD>(key)) * 16);
      waddr[i][1] = row + (((2 * cc + (flip ? 0 : 1)) ^ kv_swz<HD>(key)) * 16);
      caddr[i] = smem_lds + p * 1024 + lane * 16;
    }
  }
  // K row reads (A operand of S^T): key qq of a 32-key block, chunk 2 ks + h
  int kaddr[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) kaddr[ks] = qq * ROWB + (((2 * ks + h) ^ kv_swz<HD>(qq)) * 16);
  // V transposed reads (A operand of O^T): see attn_prefill2_kernel
  const int gi = lane >> 4, qr = (lane & 15) >> 2, pc = lane & 3;
  int vaddr[DB][2];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = 4 * h + qr + 8 * u;
      const int chunk = 4 * db + 2 * (gi & 1) + (pc >> 1);
      vaddr[db][u] = key * ROWB + ((chunk ^ kv_swz<HD>(key)) * 16) + 8 * (pc & 1);
    }

  const int passes = QB == 1 ? 2 : 1;
  for (int pass = 0; pass < passes; ++pass) {
    // ---- which query block this wave owns (attn_prefill2_kernel's complementary pairs) ---------------
    int blk_q, pair;
    bool blk_ok;
    if (QB == 1) {
      pair = blockIdx.x;
      blk_q = pass == 0 ? nblk - 1 - pair : pair;
      blk_ok = pair < npair && !(pass == 1 && pair == nblk - 1 - pair);
    } else {
      pair = (int)blockIdx.x * (QB >> 1) + (slot >> 1);
      blk_q = (slot & 1) ? nblk - 1 - pair : pair;
      blk_ok = pair < npair && !((slot & 1) && pair == nblk - 1 - pair);
    }
    const int q0 = blk_q * 32;
    const bool active = blk_ok && head_ok;
    const int p_first = q_pos0 + min(q0, T - 1), p_last = q_pos0 + min(q0 + 31, T - 1);
    const int nt_wave = active ? p_last / TK + 1 : 0;
    int wg_pair0 = QB == 1 ? (int)blockIdx.x : (int)blockIdx.x * (QB >> 1);
    int wg_blk = QB == 1 ? (pass == 0 ? nblk - 1 - wg_pair0 : wg_pair0) : nblk - 1 - wg_pair0;   // heaviest block of the work-group
    wg_blk = max(min(wg_blk, nblk - 1), 0);
    const int nt = (q_pos0 + min(wg_blk * 32 + 31, T - 1)) / TK + 1;

    // ---- Q fragments (B operand of S^T): Q[q0 + qq][16 ks + 8 h ..] ---------------------------------
    const int qi = min(q0 + qq, T - 1);
    const int qpos = q_pos0 + qi;
    u32x4_t qf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      qf[ks] = active ? *reinterpret_cast<const u32x4_t*>(q + ((size_t)qi * nh + head) * HD + ks * 16 + h * 8) : u32x4_t{0, 0, 0, 0};

    f32x16_t o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m_used = -INFINITY, lsum = 0.f;

    // Block ids (scalar loads) are fetched one tile ahead of the DMAs that use them, as in attn_prefill2_kernel.
    int pf_blk[PW], pf_off[PW];
    auto fetch_ids = [&](int t) {
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int k0 = min(t * TK + ((wave + NW * i) % NP) * KPP, last_piece_key);   // past the context: the last piece again (masked by position)
        int bi;
        if (bs_shift >= 0) { bi = k0 >> bs_shift; pf_off[i] = k0 & (bs - 1); }
        else { bi = k0 / bs; pf_off[i] = k0 - bi * bs; }
        pf_blk[i] = block_table[bi];
      }
    };
    auto issue = [&](int st) {                  // the tile whose ids fetch_ids loaded last
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = wave + NW * i;
        const size_t row = ((size_t)pf_blk[i] * nkv + kvh) * bs + pf_off[i];
        glds16((p >= NP ? vpool : kpool) + row * HD + lane * 16, smem + st * CSTAGE + p * 1024);
      }
    };
    // tile u: wave-private code stage -> the work-group's image[u & 1].  Tiles u + 1 and u + 2 stay in flight.
    int st_issue = 0, st_widen = 0;
    auto widen = [&](int u) {
      if (u + 2 < nt) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PW) : "memory");
      } else if (u + 1 < nt) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PW) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      const unsigned coff = st_widen * CSTAGE, ioff = (u & 1) * ISTAGE;
      st_widen = st_widen == NSTAGE - 1 ? 0 : st_widen + 1;
      u32x4_t cw[PW];
#pragma unroll
      for (int i = 0; i < PW; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(cw[i]) : "v"(caddr[i] + coff) : "memory");
      // (0, not counted: scalar loads share the counter and return out of order)
      if constexpr (PW == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cw[0]), "+v"(cw[PW - 1]) : : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cw[0]) : : "memory");
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const bf16x8_t lo = decode8<MI_W_F8E4M3>(cw[i][0], cw[i][1]), hi = decode8<MI_W_F8E4M3>(cw[i][2], cw[i][3]);
        asm volatile("ds_write_b128 %0, %1" ::"v"(waddr[i][0] + ioff), "v"(flip ? hi : lo) : "memory");
        asm volatile("ds_write_b128 %0, %1" ::"v"(waddr[i][1] + ioff), "v"(flip ? lo : hi) : "memory");
      }
    };

    fetch_ids(0);
    issue(0);
    if (nt > 1) { fetch_ids(1); issue(1); }
    if (nt > 2) { fetch_ids(2); issue(2); }
    fetch_ids(3);                              // st_issue: 3 % NSTAGE = 0
    // (the Q fragments' wait in front of the loop, not as a vmcnt(0) inside it: see attn_prefill2_kernel)
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) asm volatile("" : "+v"(qf[ks]));
    widen(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();              // image[0] holds tile 0 (and the previous pass is done with both images)
    for (int t = 0; t < nt; ++t) {
      if (t + 3 < nt) {                          // into the stage tile t left when it was widened; ids one tile ahead
        issue(st_issue);
        st_issue = st_issue == NSTAGE - 1 ? 0 : st_issue + 1;
        fetch_ids(t + 4);
      }
      const unsigned char* Kst = img + (t & 1) * ISTAGE;
      const unsigned char* Vst = Kst + KIMG;
      if (t < nt_wave) {                         // wave-uniform: else the tile lies in this block's future (or the slot is idle)
      // ---- S^T = K . Q^T : two 32-key blocks, K fragments requested one block ahead of their MFMAs ----
      f32x16_t sc[2];
      {
        bf16x8_t kf[KSTEPS];
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) kf[ks] = *reinterpret_cast<const bf16x8_t*>(Kst + kaddr[ks]);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[b][r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KSTEPS; ++ks) {
            sc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], __builtin_bit_cast(bf16x8_t, qf[ks]), sc[b], 0, 0, 0);
            if (b == 0) kf[ks] = *reinterpret_cast<const bf16x8_t*>(Kst + 32 * ROWB + kaddr[ks]);
          }
        }
        __builtin_amdgcn_sched_group_barrier(0x100, KSTEPS, 0);
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
      }
      // ---- online softmax: this lane holds 32 scores of query qq (keys (r & 3) + 8 (r >> 2) + 4 h of each block) ----
      const bool need_mask = t * TK + TK - 1 > p_first;
      if (need_mask) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (t * TK + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h > qpos) sc[b][r] = -INFINITY;
      }
      float mx = sc[0][0];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[b][r]);
      {
        const f32x2_t sw = swap32_pair(mx);
        mx = fmaxf(sw[0], sw[1]);
      }
      const float ms = mx * score_scale;         // key 0 is visible to every query: finite from the first tile on
      const bool moved = ms > m_used + kDeferLog2;
      if (__any(moved)) {
        const float mn = moved ? ms : m_used;
        const float alpha = moved ? fexp2(m_used - mn) : 1.f;   // exp2(-inf) = 0 on the first tile
        m_used = mn;
        lsum *= alpha;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      }
      // ---- p = exp2(s - m) packed to bf16 = the B operands of O^T += V^T . P^T; transposed V fragments by inline asm,
      // kVAhead MFMAs ahead of their use, completion counted by hand inside the fenced window ----
      constexpr int NPV = 4 * DB;               // MFMAs: (b, s2) outer, d-block inner
      constexpr int kVAhead = 4;
      s16x4_t vlo[NPV], vhi[NPV];
      unsigned vbase[DB][2];
      const unsigned vst_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)Vst;
#pragma unroll
      for (int db = 0; db < DB; ++db) { vbase[db][0] = vst_lds + vaddr[db][0]; vbase[db][1] = vst_lds + vaddr[db][1]; }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the widening's writes, the block ids, the K fragments: nothing outstanding
      __builtin_amdgcn_sched_barrier(0);                   // ... and nothing moves into the window
#define MI_VREAD(i_)                                                                                                         \
      do {                                                                                                                   \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vlo[i_]) : "v"(vbase[(i_) % DB][0]), "n"(16 * ((i_) / DB) * ROWB)); \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vhi[i_]) : "v"(vbase[(i_) % DB][1]), "n"(16 * ((i_) / DB) * ROWB)); \
      } while (0)
      MI_VREAD(0); MI_VREAD(1); MI_VREAD(2); MI_VREAD(3);
      static_assert(kVAhead == 4, "the prefetch above is written out for 4");
      bf16x8_t pb[4];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float pv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          pv[r] = fexp2(fmaf(sc[b][r], score_scale, -m_used));   // masked: exp2(-inf) = 0
          lsum += pv[r];
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          union { uint32_t w[4]; bf16x8_t v; } pk;
#pragma unroll
          for (int k = 0; k < 4; ++k) pk.w[k] = pack_bf16x2(pv[8 * s2 + 2 * k], pv[8 * s2 + 2 * k + 1]);
          pb[2 * b + s2] = pk.v;
        }
      }
#define MI_PV(i_)                                                                                                            \
      do {                                                                                                                   \
        constexpr int issued = 2 * ((i_) + kVAhead < NPV ? (i_) + kVAhead : NPV);                                            \
        asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(vlo[i_]), "+v"(vhi[i_]) : "n"(issued - 2 * ((i_) + 1)));               \
        const s16x4_t lo = vlo[i_], hi = vhi[i_];                                                                            \
        const bf16x8_t a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                                         \
        o[(i_) % DB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb[(i_) / DB], o[(i_) % DB], 0, 0, 0);                     \
        if constexpr ((i_) + kVAhead < NPV) MI_VREAD((i_) + kVAhead);                                                        \
      } while (0)
      MI_PV(0); MI_PV(1); MI_PV(2); MI_PV(3); MI_PV(4); MI_PV(5); MI_PV(6); MI_PV(7);
      if constexpr (NPV == 16) { MI_PV(8); MI_PV(9); MI_PV(10); MI_PV(11); MI_PV(12); MI_PV(13); MI_PV(14); MI_PV(15); }
#undef MI_PV
#undef MI_VREAD
      __builtin_amdgcn_sched_barrier(0);
      }
      if (t + 1 < nt) widen(t + 1);              // under the tail of this tile's P.V MFMAs
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's share of image[(t + 1) & 1] is written
      __builtin_amdgcn_s_barrier();            // tile t + 1 is whole; everyone is done reading tile t
    }
    // ---- epilogue: (O^T[d][q] / l) v_scale -> out[q][head][d], 16-byte stores by one v_permlane32_swap per pair of groups
    {
      const f32x2_t sw = swap32_pair(lsum);
      lsum = sw[0] + sw[1];
    }
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    const bool st_ok = active && q0 + qq < T;
    uint16_t* orow = out + ((size_t)(q0 + qq) * nh + head) * HD;
    auto fin = [&](float x) { return x * inv * v_scale; };
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int k2 = 0; k2 < 4; k2 += 2) {      // dim groups k2, k2 + 1: dims 32 db + 8 k + 4 h + (0..3)
        uint32_t a0 = pack_bf16x2(fin(o[db][4 * k2 + 0]), fin(o[db][4 * k2 + 1]));
        uint32_t a1 = pack_bf16x2(fin(o[db][4 * k2 + 2]), fin(o[db][4 * k2 + 3]));
        uint32_t b0 = pack_bf16x2(fin(o[db][4 * k2 + 4]), fin(o[db][4 * k2 + 5]));
        uint32_t b1 = pack_bf16x2(fin(o[db][4 * k2 + 6]), fin(o[db][4 * k2 + 7]));
        const auto x = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto y = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        const u32x4_t v = {x[0], y[0], x[1], y[1]};
        if (st_ok) *reinterpret_cast<u32x4_t*>(orow + 32 * db + 8 * (k2 + h)) = v;
      }
    // (no barrier here: the loop's last one covers the images, and the code ring is wave-private)
  }
}

// ---- launch ------------------------------------------------------------------------------------------------------
// 8 waves = (8 / Gp) query blocks x Gp heads; blocks in complementary pairs
struct PrefillLaunch {
  int G, Gp, nblk, bs_shift;   // bs_shift: log2(block_size), -1 when it is no power of two
  dim3 grid;
  float scale_log2e;
};
static int prefill_launch_geometry(int T, int q_pos0, int block_size, int nh, int nkv, int hd, PrefillLaunch* g) {
  MI_CHECK(hd == 64 || hd == 128, "attention: head_dim must be 64 or 128");
  MI_CHECK(T >= 1 && q_pos0 >= 0, "attention: bad T / q_pos0");
  MI_CHECK(nh % nkv == 0 && nh / nkv <= 8, "attention: q heads per kv head must be 1..8");
  // mi_ctx_create holds max_model_len to the same bound, so a context that was created never meets this
  MI_CHECK(ceil_div(q_pos0 + T, block_size) <= kPrefillMaxBlocks, "attention: context spans more than 4096 blocks");
  g->G = nh / nkv;
  g->Gp = g->G <= 1 ? 1 : (g->G <= 2 ? 2 : (g->G <= 4 ? 4 : 8));
  g->nblk = ceil_div(T, 32);
  const int npair = (g->nblk + 1) / 2, qb = 8 / g->Gp;
  g->bs_shift = -1;
  for (int sh = 4; sh < 20; ++sh) if ((1 << sh) == block_size) g->bs_shift = sh;
  g->grid = dim3(ceil_div(npair, qb >= 2 ? qb / 2 : 1), nkv);
  g->scale_log2e = 1.4426950408889634f / sqrtf((float)hd);
  return MI_OK;
}

// Sliding window: 8 waves = (8 / Gp) ADJACENT query blocks x Gp heads, grid ceil(nblk / (8 / Gp)) x nkv.
// Blocks per work-group: a block's band is (W + 95) / 64 tiles wherever it lies, so every work-group carries the same load
// and nothing is gained by pairing; what the count decides is how much of the ring a wave sits out.  With QB adjacent
// blocks the ring walks (W + 32 QB + 63) / 64 tiles and a wave multiplies (W + 95) / 64 of them: at QB = 2 (4 q heads per
// kv head, the common GQA shape) one tile in 66 at W 4096 is skipped, at QB = 8 (MHA) 4 in 69 -- a skipped tile costs a
// wave its DMA share and a barrier, no MFMA.  Fewer blocks than 8 / Gp would leave waves of the work-group idle for the
// whole launch (the head slots are fixed by Gp), more would need a second pass over a ring that no longer overlaps: so
// 8 / Gp it is, the slot layout of the unwindowed kernel.
static int prefill_sw_launch_geometry(int T, int q_pos0, int block_size, int nh, int nkv, int hd, PrefillLaunch* g) {
  MI_TRY_A(prefill_launch_geometry(T, q_pos0, block_size, nh, nkv, hd, g));
  g->grid = dim3(ceil_div(g->nblk, 8 / g->Gp), nkv);
  return MI_OK;
}

int launch_attn_prefill(const uint16_t* q, int T, int q_pos0, const uint16_t* kpool, const uint16_t* vpool,
                        int block_size, const int32_t* block_table, int nh, int nkv, int hd, uint16_t* out,
                        hipStream_t s, int window) {
  MI_CHECK(window >= 0, "attention: the sliding window must be >= 0 (0 = none)");
  PrefillLaunch g;
  if (window > 0 && q_pos0 + T > window) {   // else the window covers every key: the unwindowed kernel and geometry
    MI_TRY_A(prefill_sw_launch_geometry(T, q_pos0, block_size, nh, nkv, hd, &g));
    auto launch_sw = [&](auto hd_c) -> int {
      constexpr int HD = decltype(hd_c)::value, lds = attn_prefill_lds<HD>();
      MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_prefill2_kernel<HD, 8, true>), lds));
      hipLaunchKernelGGL((attn_prefill2_kernel<HD, 8, true>), g.grid, dim3(512), lds, s, q, T, q_pos0, kpool, vpool, block_size,
                         g.bs_shift, block_table, nh, nkv, g.G, g.Gp, g.nblk, out, g.scale_log2e, window);
      MI_HIP(hipGetLastError());
      return MI_OK;
    };
    return hd == 128 ? launch_sw(std::integral_constant<int, 128>{}) : launch_sw(std::integral_constant<int, 64>{});
  }
  MI_TRY_A(prefill_launch_geometry(T, q_pos0, block_size, nh, nkv, hd, &g));
  auto launch = [&](auto hd_c) -> int {
    constexpr int HD = decltype(hd_c)::value, lds = attn_prefill_lds<HD>();
    MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_prefill2_kernel<HD, 8>), lds));
    hipLaunchKernelGGL((attn_prefill2_kernel<HD, 8>), g.grid, dim3(512), lds, s, q, T, q_pos0, kpool, vpool, block_size,
                       g.bs_shift, block_table, nh, nkv, g.G, g.Gp, g.nblk, out, g.scale_log2e);
    MI_HIP(hipGetLastError());
    return MI_OK;
  };
  return hd == 128 ? launch(std::integral_constant<int, 128>{}) : launch(std::integral_constant<int, 64>{});
}

int launch_attn_prefill_f8(const uint16_t* q, int T, int q_pos0, const uint8_t* kpool, const uint8_t* vpool,
                           int block_size, const int32_t* block_table, int nh, int nkv, int hd, float k_scale,
                           float v_scale, uint16_t* out, hipStream_t s) {
  MI_CHECK(block_size >= 16 && block_size % 16 == 0, "attention: block_size must be a multiple of 16");   // a DMA piece (8 / 16 keys) never straddles blocks
  PrefillLaunch g;
  MI_TRY_A(prefill_launch_geometry(T, q_pos0, block_size, nh, nkv, hd, &g));
  MI_CHECK(k_scale > 0.f && v_scale > 0.f, "attention: the FP8 KV scales must be positive");
  auto launch = [&](auto hd_c) -> int {
    constexpr int HD = decltype(hd_c)::value, lds = attn_prefill_f8_lds<HD>();
    MI_TRY_A(ensure_dynamic_lds(reinterpret_cast<const void*>(attn_prefill_f8_kernel<HD, 8>), lds));
    hipLaunchKernelGGL((attn_prefill_f8_kernel<HD, 8>), g.grid, dim3(512), lds, s, q, T, q_pos0, kpool, vpool, block_size,
                       g.bs_shift, block_table, nh, nkv, g.G, g.Gp, g.nblk, out, g.scale_log2e * k_scale, v_scale);
    MI_HIP(hipGetLastError());
    return MI_OK;
  };
  return hd == 128 ? launch(std::integral_constant<int, 128>{}) : launch(std::integral_constant<int, 64>{});
}

// =====================================================================================
// standalone KV write (the model path writes K/V from the QKV epilogue instead)
// =====================================================================================
__global__ void kv_write_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                const int64_t* __restrict__ slots, int nkv, int hd, uint16_t* __restrict__ kpool,
                                uint16_t* __restrict__ vpool, int bs) {
  const int t = blockIdx.x;
  const long slot = slots[t];
  if (slot < 0) return;
  const int blk = (int)(slot / bs), off = (int)(slot % bs);
  const int chunks = nkv * hd / 8;
  for (int i = threadIdx.x; i < chunks; i += blockDim.x) {
    const int head = (i * 8) / hd, d = (i * 8) % hd;
    const size_t dst = (((size_t)blk * nkv + head) * bs + off) * hd + d;
    *reinterpret_cast<uint4*>(kpool + dst) = *reinterpret_cast<const uint4*>(k + (size_t)t * nkv * hd + i * 8);
    *reinterpret_cast<uint4*>(vpool + dst) = *reinterpret_cast<const uint4*>(v + (size_t)t * nkv * hd + i * 8);
  }
}

int launch_kv_write(const uint16_t* k, const uint16_t* v, const int64_t* slots, int T, int nkv, int hd,
                    uint16_t* kpool, uint16_t* vpool, int block_size, hipStream_t s) {
  MI_CHECK(hd % 8 == 0, "kv_write: head_dim % 8 == 0 required");
  if (T == 0) return MI_OK;
  hipLaunchKernelGGL(kv_write_kernel, dim3(T), dim3(128), 0, s, k, v, slots, nkv, hd, kpool, vpool, block_size);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// ---- FP8 pool: the write rule of mi_common.h (kv_quant4) per 4 values, one 4-byte store each --------------------
__global__ void kv_write_f8_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                   const int64_t* __restrict__ slots, int nkv, int hd, uint8_t* __restrict__ kpool,
                                   uint8_t* __restrict__ vpool, int bs, float k_inv, float v_inv) {
  const int t = blockIdx.x;
  const long slot = slots[t];
  if (slot < 0) return;
  const int blk = (int)(slot / bs), off = (int)(slot % bs);
  const int quads = nkv * hd / 4;
  for (int i = threadIdx.x; i < quads; i += blockDim.x) {
    const int head = (i * 4) / hd, d = (i * 4) % hd;
    const size_t dst = (((size_t)blk * nkv + head) * bs + off) * hd + d;
    *reinterpret_cast<uint32_t*>(kpool + dst) = kv_quant4(*reinterpret_cast<const uint2*>(k + (size_t)t * nkv * hd + i * 4), k_inv);
    *reinterpret_cast<uint32_t*>(vpool + dst) = kv_quant4(*reinterpret_cast<const uint2*>(v + (size_t)t * nkv * hd + i * 4), v_inv);
  }
}

int launch_kv_write_f8(const uint16_t* k, const uint16_t* v, const int64_t* slots, int T, int nkv, int hd, uint8_t* kpool,
                       uint8_t* vpool, int block_size, float k_scale, float v_scale, hipStream_t s) {
  MI_CHECK(hd % 16 == 0, "kv_write_f8: head_dim % 16 == 0 required");
  MI_CHECK(k_scale > 0.f && v_scale > 0.f, "kv_write_f8: FP8 KV scales must be positive");
  if (T == 0) return MI_OK;
  hipLaunchKernelGGL(kv_write_f8_kernel, dim3(T), dim3(128), 0, s, k, v, slots, nkv, hd, kpool, vpool, block_size,
                     1.0f / k_scale, 1.0f / v_scale);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// =====================================================================================
// per-head QK-norm + RoPE + q buffer / KV-pool write (Qwen3)
// =====================================================================================
// qkv [T, (nh + 2 nkv) * HD] fp32 is the fused projection as EPI_F32 leaves it: q and k heads pair-interleaved
// (column 2i <- d = i, 2i + 1 <- d = i + HD/2), V plain.  A lane owns one float4 of one (token, head) row = two
// rotation pairs, the unit of the 8-byte q / K stores and of kv_quant4; a row is HD/4 lanes (32 or 16), a wave holds
// 2 or 4 rows.  The (token, head) rows are flattened over the grid, so an odd head count (7 q + 2 kv) leaves no lane
// group idle and a wave may hold the last heads of one token and the first of the next: every lane group reads its
// own pos / slot.  Loads, in request order: pos + slot, the row and its gain, then cos / sin (they hang off pos, not
// off the reduction); the sum of squares goes through DPP inside the row's lanes.  No LDS, no barrier.
//   q, k:  z = (y * rsqrtf(sum(y^2) / HD + eps)) * g -> RoPE in fp32 (as epilogue_store<EPI_QKV>) -> bf16 (RNE)
//   v:     bf16 (RNE)
// An all-zero row (a padding q head of a TP shard) has r = rsqrtf(eps), finite: it stays zero.
template <bool F8, int HD>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_kernel(
    const float* __restrict__ qkv, const float* __restrict__ gq, const float* __restrict__ gk,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ slots, int rows, int nh, int nkv, float eps,
    const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, uint16_t* __restrict__ q_out,
    void* __restrict__ kpool, void* __restrict__ vpool, int nslots, int bs, float k_inv, float v_inv) {
  constexpr int LPR = HD / 4;                       // lanes per (token, head) row
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = tid / LPR, c = (tid % LPR) * 4;   // c: first of the lane's four columns inside the head
  const bool live = row < rows;                     // whole lane groups are live or not
  const int nht = nh + 2 * nkv;
  const int t = live ? row / nht : 0, h = live ? row % nht : 0;
  const bool is_q = h < nh, is_qk = h < nh + nkv;
  const int p = max(pos[t], 0), slot = slots[t];
  float4 y = make_float4(0.f, 0.f, 0.f, 0.f), g = y;
  float2 cs = make_float2(1.f, 1.f), sn = make_float2(0.f, 0.f);
  if (live) y = *reinterpret_cast<const float4*>(qkv + ((size_t)t * nht + h) * HD + c);
  if (live && is_qk) {
    g = *reinterpret_cast<const float4*>((is_q ? gq : gk) + c);
    cs = *reinterpret_cast<const float2*>(rope_cos + (size_t)p * (HD / 2) + (c >> 1));
    sn = *reinterpret_cast<const float2*>(rope_sin + (size_t)p * (HD / 2) + (c >> 1));
  }
  float ss = group_sum<16>(y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w);
  if (LPR == 32) ss += __shfl_xor(ss, 16);
  if (!live) return;
  if (is_qk) {
    const float r = rsqrtf(ss * (1.0f / HD) + eps);
    const float z0 = (y.x * r) * g.x, z1 = (y.y * r) * g.y, z2 = (y.z * r) * g.z, z3 = (y.w * r) * g.w;
    y.x = z0 * cs.x - z1 * sn.x; y.y = z1 * cs.x + z0 * sn.x;
    y.z = z2 * cs.y - z3 * sn.y; y.w = z3 * cs.y + z2 * sn.y;
  }
  const uint2 packed = make_uint2(pack_bf16x2(y.x, y.y), pack_bf16x2(y.z, y.w));
  if (is_q) {
    *reinterpret_cast<uint2*>(q_out + ((size_t)t * nh + h) * HD + c) = packed;
  } else if (slot >= 0 && slot < nslots) {
    const int head = is_qk ? h - nh : h - nh - nkv;
    const size_t at = (((size_t)(slot / bs) * nkv + head) * bs + slot % bs) * HD + c;
    if (F8) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(is_qk ? kpool : vpool) + at) = kv_quant4(packed, is_qk ? k_inv : v_inv);
    else *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(is_qk ? kpool : vpool) + at) = packed;
  }
}

int launch_qk_norm_rope_kv(const float* qkv, const float* gq, const float* gk, const int32_t* pos, const int32_t* slots,
                           int T, int nh, int nkv, int hd, float eps, const float* rope_cos, const float* rope_sin,
                           uint16_t* q_out, void* kpool, void* vpool, int num_blocks, int block_size, bool f8, float k_scale,
                           float v_scale, hipStream_t s) {
  MI_CHECK(hd == 64 || hd == 128, "qk_norm_rope_kv: head_dim must be 64 or 128");
  MI_CHECK(T >= 0 && nh >= 1 && nkv >= 1 && num_blocks >= 1 && block_size >= 1, "qk_norm_rope_kv: bad geometry");
  MI_CHECK((size_t)T * (nh + 2 * nkv) * (hd / 4) < ((size_t)1 << 31) && (size_t)num_blocks * block_size < ((size_t)1 << 31),
           "qk_norm_rope_kv: too many rows / slots");
  MI_CHECK(!f8 || (k_scale > 0.f && v_scale > 0.f), "qk_norm_rope_kv: FP8 KV scales must be positive");
  if (T == 0) return MI_OK;
  const int rows = T * (nh + 2 * nkv), lanes = rows * (hd / 4);
  // a token-generation step is a few hundred rows: one wave per work-group spreads them over the CUs; a context-encoding
  // bucket streams through 4-wave work-groups
  const int block = lanes >= 64 * 1024 ? 256 : 64;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(ceil_div(lanes, block)), dim3(block), 0, s, qkv, gq, gk, pos, slots, rows, nh, nkv, eps,
                       rope_cos, rope_sin, q_out, kpool, vpool, num_blocks * block_size, block_size,
                       f8 ? 1.0f / k_scale : 1.f, f8 ? 1.0f / v_scale : 1.f);
  };
  if (hd == 128) f8 ? launch(qk_norm_rope_kv_kernel<true, 128>) : launch(qk_norm_rope_kv_kernel<false, 128>);
  else f8 ? launch(qk_norm_rope_kv_kernel<true, 64>) : launch(qk_norm_rope_kv_kernel<false, 64>);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

// ---- FP8 pool -> bf16 staging pool for context encoding ---------------------------------------------------------
// The blocks of ONE sequence, in block-table order: staged [2][nblk][nkv][bs][hd] bf16 = bf16_rne(float(code) * scale).
// A (block, all heads) range is contiguous in both pools, so a thread widens 16 codes (one 16-byte load, two 16-byte
// stores); grid (chunks of a block, nblk, K / V).  Whole blocks are staged: the tail of the last one is finite pool
// content that the attention kernel masks.
__global__ __launch_bounds__(256) void kv_dequant_gather_kernel(const uint8_t* __restrict__ pool, size_t half_bytes,
                                                                int num_blocks, int blk_bytes,
                                                                const int32_t* __restrict__ block_table, int nblk,
                                                                float k_scale, float v_scale, uint16_t* __restrict__ staged) {
  const int chunk = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, kv = blockIdx.z;
  if (chunk * 16 >= blk_bytes) return;
  const int blk = min(max(block_table[i], 0), num_blocks - 1);
  const float scale = kv ? v_scale : k_scale;
  const u32x4_t cw = *reinterpret_cast<const u32x4_t*>(pool + kv * half_bytes + (size_t)blk * blk_bytes + (size_t)chunk * 16);
  uint16_t* dst = staged + ((size_t)kv * nblk + i) * blk_bytes + (size_t)chunk * 16;
  u32x4_t lo, hi;
  lo[0] = kv_dequant2_bf16(cw[0], false, scale); lo[1] = kv_dequant2_bf16(cw[0], true, scale);
  lo[2] = kv_dequant2_bf16(cw[1], false, scale); lo[3] = kv_dequant2_bf16(cw[1], true, scale);
  hi[0] = kv_dequant2_bf16(cw[2], false, scale); hi[1] = kv_dequant2_bf16(cw[2], true, scale);
  hi[2] = kv_dequant2_bf16(cw[3], false, scale); hi[3] = kv_dequant2_bf16(cw[3], true, scale);
  *reinterpret_cast<u32x4_t*>(dst) = lo;
  *reinterpret_cast<u32x4_t*>(dst + 8) = hi;
}

int launch_kv_dequant_gather(const uint8_t* pool, int num_blocks, int block_size, const int32_t* block_table, int MB,
                             int kv_len, int nkv, int hd, float k_scale, float v_scale, uint16_t* staged, hipStream_t s,
                             int first_blk) {
  MI_CHECK(hd % 16 == 0 && num_blocks >= 1 && block_size >= 1 && nkv >= 1, "kv_dequant_gather: bad pool geometry");
  MI_CHECK(kv_len >= 1 && ceil_div(kv_len, block_size) <= MB, "kv_dequant_gather: block_table narrower than the context");
  const int nblk = ceil_div(kv_len, block_size), blk_bytes = nkv * block_size * hd;
  MI_CHECK(first_blk >= 0 && first_blk < nblk, "kv_dequant_gather: first block outside the context");
  // blocks first_blk .. nblk - 1 keep their place in the staged pool: the kernel sees the table and the staged pool from
  // first_blk on, with nblk still the stride between the K and the V part
  hipLaunchKernelGGL(kv_dequant_gather_kernel, dim3(ceil_div(blk_bytes / 16, 256), nblk - first_blk, 2), dim3(256), 0, s, pool,
                     (size_t)num_blocks * blk_bytes, num_blocks, blk_bytes, block_table + first_blk, nblk, k_scale, v_scale,
                     staged + (size_t)first_blk * blk_bytes);
  MI_HIP(hipGetLastError());
  return MI_OK;
}

}  // namespace mi
