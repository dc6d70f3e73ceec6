// Model of the fat-wave Gram matvec's inner loop on v_mfma_f32_16x16x32_f16 (round 5), as an instruction-stream and data-toggling
// model on random data -- NOT a correct matvec.  One wave per SIMD (256-thread workgroups, 512 registers).
//
// Unit of work = 16 rows x 32 columns of the Gram matrix x 64 probes: 2 distance MFMAs (the two 16-column halves; inner dimension
// 3 (d + 2) <= 32 is ONE k-step), 8 kernel entries per lane -> 8 v_exp, 4 v_cvt_pk (hi pairs), 4 v_fma_mixlo + 4 v_fma_mixhi (lo
// pairs), 12 contraction MFMAs (4 probe groups of 16 x {hi hi, hi lo, lo hi}).  14 MFMA slots of 16 cycles; an MFMA holds the
// vector issue for 8 of them (MI355X_MICROARCH.md), the 20 VALU instructions cost 8 x 8 + 12 x 4 = 112 = 14 x 8: the unit is
// EXACTLY issue-balanced, every slot carries 8 issue cycles of VALU (one v_exp, or two 4-cycle instructions).
// A 64-column tile = 16 units (2 column halves x 8 row tiles of the wave's 128 rows).
//
// Variants (bit mask VAR): 1 chain on; 2 the three products of an accumulator back to back (else product-major: 4 different
// accumulators between two MFMAs on the same one); 4 LDS fragment reads on; 8 LDS-DMA of the tile images + barrier per tile;
// 16 the 32x32x16 reference loop of tools/shape_bench.hip (SHAPE 0) instead; 512 the tile loop of k_rbf_fat_apply16 as shipped: two
// tiles per iteration, the LDS buffer a constant of the code (every offset an immediate, nothing carried across the back edge).
// The like-for-like row: the 32x32x16 loop (k32) has the fragment reads of k_rbf_fat_apply in every form; with DMA = 1 it also has
// the kernel's LDS-DMA (21 pieces of 1 KiB per 64-column tile = 8 blocks, requested in block 5) and its one barrier per tile
// (behind block 4).  That row, not the bare chain row, is what the full 16x16x32 row (VAR 1 + 4 + 8) compares with.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// one micro-step of the split chain of a unit (8 entries w[0..7] = two floatx4): t = 0 exp2 of entry i; 1 hi pair i; 2 lo half of entry i
__device__ __forceinline__ void chain16(floatx4 (&w)[2], half8& ah, half8& al, unsigned (&lp)[4], int t, int i) {
  if (t == 0) {
    w[i >> 2][i & 3] = __builtin_amdgcn_exp2f(w[i >> 2][i & 3]);
  } else if (t == 1) {
    const half2v h = {(_Float16)w[i >> 1][(2 * i) & 3], (_Float16)w[i >> 1][(2 * i + 1) & 3]};
    ah[2 * i] = h[0];
    ah[2 * i + 1] = h[1];
  } else {
    const int pr = i >> 1;
    const half2v h = {ah[2 * pr], ah[2 * pr + 1]};
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    if ((i & 1) == 0) {
      asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lp[pr]) : "v"(hb), "v"(w[i >> 2][i & 3]));
    } else {
      asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lp[pr]) : "v"(hb), "v"(w[i >> 2][i & 3]));
      const half2v l = __builtin_bit_cast(half2v, lp[pr]);
      al[2 * pr] = l[0];
      al[2 * pr + 1] = l[1];
    }
  }
}

// the placement table of a unit's chain behind the 14 slots of the unit BEFORE it
struct Tab16 { int e[8], h[4], m[8]; };
// T0: exps behind slots 0-7, then pairs of 4-cycle steps: every slot carries exactly 8 issue cycles
constexpr Tab16 kT0 = {{0, 1, 2, 3, 4, 5, 6, 7}, {8, 8, 9, 9}, {10, 11, 10, 11, 12, 13, 12, 13}};
// T1: interleaved: exp slots and pair slots alternate (0 e, 1 e, 2 e, 3 e, 4 hh, 5 e, 6 e ...), same per-slot cost
constexpr Tab16 kT1 = {{0, 1, 2, 3, 5, 6, 8, 9}, {4, 4, 10, 10}, {7, 11, 7, 11, 12, 13, 12, 13}};

template <int VAR>
__global__ __launch_bounds__(256, 1) void k16(const _Float16* __restrict__ rnd, const _Float16* __restrict__ img, float* out, long long* cyc, int tiles) {
  constexpr bool CHAIN = VAR & 1, SAMEACC = VAR & 2, LDSRD = VAR & 4, DMA = VAR & 8, TAB1 = (VAR & 32) != 0;
  constexpr bool TWO = (VAR & 512) != 0;
  constexpr bool NOEXP = (VAR & 64) != 0, NOCVT = (VAR & 128) != 0, NOMIX = (VAR & 256) != 0;  // parts of the chain compiled out
  constexpr Tab16 T = TAB1 ? kT1 : kT0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  // two tile buffers of 20 KiB: [16 probe fragments | 4 column-operand fragments], each fragment 1 KiB in lane order
  for (int i = tid; i < 40960 / 2; i += 256) {
    const _Float16 v = rnd[(blockIdx.x * 977 + i) % (1 << 20)];
    const int piece = (i / 512) % 20;
    reinterpret_cast<_Float16*>(smem)[i] = piece >= 16 ? (_Float16)((float)v * (1.f / 12000.f)) : v;
  }
  __syncthreads();
  float agpr_seed = 0.f;
  asm volatile("; agpr" : "+a"(agpr_seed));
  floatx4 acc[32];
  for (int q = 0; q < 32; ++q)
    for (int r = 0; r < 4; ++r) acc[q][r] = 0.f;
  acc[0][0] = agpr_seed;
  half8 vf[2][8];   // probe fragments [column-half parity][pg * 2 + hl]
  half8 aj[2][2];   // column operand [column-half parity][16-column tile]
  half8 bi[8];      // row operand of the wave's 8 row tiles
  half8 ah[2], al[2];
  unsigned lp[4] = {0, 0, 0, 0};
  floatx4 wr[4][2];  // distance tiles: ring of four units
  const char* base = smem + lane * 16;
  for (int q = 0; q < 8; ++q) {
    vf[0][q] = *reinterpret_cast<const half8*>(base + q * 1024);
    vf[1][q] = *reinterpret_cast<const half8*>(base + (8 + q) * 1024);
    bi[q] = *reinterpret_cast<const half8*>(base + (16 + (q & 3)) * 1024);
    for (int e = 0; e < 8; ++e) bi[q][e] = bi[q][e] * (_Float16)(1.f + 0.125f * q);
  }
  for (int q = 0; q < 2; ++q) {
    aj[0][q] = *reinterpret_cast<const half8*>(base + (16 + q) * 1024);
    aj[1][q] = *reinterpret_cast<const half8*>(base + (18 + q) * 1024);
    ah[q] = vf[0][q];
    al[q] = vf[0][q + 2];
  }
  for (int u = 0; u < 4; ++u)
    for (int q = 0; q < 8; ++q) wr[u][q >> 2][q & 3] = -0.5f * (float)(q + 1) - 1e-3f * lane - 0.1f * u;
  const long long t0 = __builtin_readcyclecounter();
  auto tile = [&](auto bc, const int t) {  // bc: the tile's buffer, t & 1 -- an int, or (TWO) a constant
    const int buf = bc;
    const char* tb = base + buf * 20480;
    auto body = [&](auto uc) {
      constexpr int u = decltype(uc)::value;   // unit of the tile: column half jh, row tile it
      constexpr int jh = u >> 3, it = u & 7;
      if (DMA && u == 10) {  // request tile t + 2 into this tile's buffer (dead since the barrier behind unit 8): 5 pieces per wave
        const char* src = reinterpret_cast<const char*>(img) + ((size_t)((t * 131 + blockIdx.x * 17) & 63)) * 20480;
#pragma unroll
        for (int c = 0; c < 5; ++c) glds16(src + (wid + 4 * c) * 1024 + lane * 16, smem + buf * 20480 + (wid + 4 * c) * 1024);
      }
#pragma unroll
      for (int slot = 0; slot < 14; ++slot) {
        __builtin_amdgcn_sched_barrier(0);
        // slots: product-major  hh0-3 (0-3), hl0-3 (4-7), d0 (8), lh0 (9), d1 (10), lh1-3 (11-13);
        //        accumulator-major (SAMEACC) pg0: hh hl lh (0-2), pg1 (3-5), pg2 (6, 7, 9), d0 (8), d1 (10), pg3 (11-13)
        if (slot == 8 || slot == 10) {
          const int q = (slot - 8) / 2;
          constexpr int u2 = (u + 2) & 15;
          asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(wr[(u + 2) & 3][q]) : "v"(aj[(u2 >> 3) & 1][q]), "v"(bi[u2 & 7]));
        } else {
          const int m = slot < 8 ? slot : (slot == 9 ? 8 : slot - 2);
          const int w = SAMEACC ? m % 3 : m / 4, pg = SAMEACC ? m / 3 : m % 4;
          acc[it * 4 + pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w == 2 ? al[u & 1] : ah[u & 1], w == 1 ? vf[jh][pg * 2 + 1] : vf[jh][pg * 2],
                                                                     acc[it * 4 + pg], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (CHAIN) {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (!NOEXP && T.e[i] == slot) chain16(wr[(u + 1) & 3], ah[(u + 1) & 1], al[(u + 1) & 1], lp, 0, i);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (!NOCVT && T.h[i] == slot) chain16(wr[(u + 1) & 3], ah[(u + 1) & 1], al[(u + 1) & 1], lp, 1, i);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (!NOMIX && T.m[i] == slot) chain16(wr[(u + 1) & 3], ah[(u + 1) & 1], al[(u + 1) & 1], lp, 2, i);
        }
        if (LDSRD) {
          // probe fragments of the next column half into the other register set: one read per unit (units it = 0 .. 7, slot 2);
          // the column operand of the column half after next: two reads in unit it = 3
          if (slot == 2) vf[jh ^ 1][it] = *reinterpret_cast<const half8*>((jh == 1 ? base + (buf ^ 1) * 20480 : tb) + ((jh ^ 1) * 8 + it) * 1024);
          if (it == 3 && slot >= 4 && slot < 6) aj[jh ^ 1][slot - 4] = *reinterpret_cast<const half8*>((jh == 1 ? base + (buf ^ 1) * 20480 : tb) + (16 + (jh ^ 1) * 2 + slot - 4) * 1024);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (DMA && u == 8) {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    };
    body(std::integral_constant<int, 0>{});
    body(std::integral_constant<int, 1>{});
    body(std::integral_constant<int, 2>{});
    body(std::integral_constant<int, 3>{});
    body(std::integral_constant<int, 4>{});
    body(std::integral_constant<int, 5>{});
    body(std::integral_constant<int, 6>{});
    body(std::integral_constant<int, 7>{});
    body(std::integral_constant<int, 8>{});
    body(std::integral_constant<int, 9>{});
    body(std::integral_constant<int, 10>{});
    body(std::integral_constant<int, 11>{});
    body(std::integral_constant<int, 12>{});
    body(std::integral_constant<int, 13>{});
    body(std::integral_constant<int, 14>{});
    body(std::integral_constant<int, 15>{});
  };
  if (TWO) {
    for (int t = 0; t + 1 < tiles; t += 2) {  // (the tile counts of main() are even)
      tile(std::integral_constant<int, 0>{}, t);
      tile(std::integral_constant<int, 1>{}, t + 1);
    }
  } else {
    for (int t = 0; t < tiles; ++t) tile(t & 1, t);
  }
  const long long t1 = __builtin_readcyclecounter();
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (tid == 0) cyc[blockIdx.x] = t1 - t0;
  float s = 0;
  for (int q = 0; q < 32; ++q)
    for (int r = 0; r < 4; ++r) s += acc[q][r];
  if (s == 12345.678f) out[0] = s;
}

// ---- the 32x32x16 loop of tools/shape_bench.hip (SHAPE 0, chain on), for the same-box reference -------------------------------------
__device__ __forceinline__ void chain_op(float (&w)[16], half8 (&ah)[2], half8 (&al)[2], unsigned (&lp)[8], int t, int i) {
  if (t == 0) {
    w[i] = __builtin_amdgcn_exp2f(w[i]);
  } else if (t == 1) {
    const half2v h = {(_Float16)w[2 * i], (_Float16)w[2 * i + 1]};
    ah[i >> 2][(i & 3) * 2] = h[0];
    ah[i >> 2][(i & 3) * 2 + 1] = h[1];
  } else {
    const int pr = i >> 1;
    const half2v h = {ah[pr >> 2][(pr & 3) * 2], ah[pr >> 2][(pr & 3) * 2 + 1]};
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    if ((i & 1) == 0) {
      asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lp[pr]) : "v"(hb), "v"(w[i]));
    } else {
      asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lp[pr]) : "v"(hb), "v"(w[i]));
      const half2v l = __builtin_bit_cast(half2v, lp[pr]);
      al[pr >> 2][(pr & 3) * 2] = l[0];
      al[pr >> 2][(pr & 3) * 2 + 1] = l[1];
    }
  }
}
template <int CHAIN, int ORDER = 0, int DMA = 0>
__global__ __launch_bounds__(256, 1) void k32(const _Float16* __restrict__ rnd, const _Float16* __restrict__ img, float* out, long long* cyc, int blocks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < 65536 / 2; i += 256) {
    const _Float16 v = rnd[(blockIdx.x * 977 + i) % (1 << 20)];
    const int piece = (i / 512) % 12;
    reinterpret_cast<_Float16*>(smem)[i] = piece >= 8 ? (_Float16)((float)v * (1.f / 12000.f)) : v;
  }
  __syncthreads();
  float agpr_seed = 0.f;
  asm volatile("; agpr" : "+a"(agpr_seed));
  floatx16 acc16[8];
  for (int q = 0; q < 8; ++q)
    for (int r = 0; r < 16; ++r) acc16[q][r] = 0.f;
  acc16[0][0] = agpr_seed;
  half8 vf[8], aj[2], bi[2];
  half8 ahc[2], alc[2], ahn[2], aln[2];
  unsigned lp[8];
  float wn[16];
  floatx16 wd16;
  const char* base = smem + lane * 16;
  for (int q = 0; q < 8; ++q) vf[q] = *reinterpret_cast<const half8*>(base + q * 1024);
  for (int q = 0; q < 2; ++q) {
    aj[q] = *reinterpret_cast<const half8*>(base + (8 + q) * 1024);
    bi[q] = *reinterpret_cast<const half8*>(base + (10 + q) * 1024);
    ahc[q] = vf[q];
    alc[q] = vf[q + 2];
    ahn[q] = vf[q];
    aln[q] = vf[q + 2];
  }
  for (int q = 0; q < 16; ++q) wn[q] = -0.5f * (float)(q + 1) - 1e-3f * lane;
  for (int q = 0; q < 8; ++q) lp[q] = 0;
  const long long t0 = __builtin_readcyclecounter();
  for (int b4 = 0; b4 < blocks / 4; ++b4) {
    const char* vb = base + (b4 & 3) * 12288;
    auto body = [&](auto bc) {
      constexpr int b = decltype(bc)::value;
      if (DMA && b == 1 && (b4 & 1)) {
        // block 5 of the tile: request the tile after next -- 5 + 16 pieces of 1 KiB, piece w, w + 4, ... by wave w -- into one of two
        // buffers BEHIND the 48 KiB the fragment reads use (the model's reads keep their data; the kernel's buffer is dead by then)
        const char* src = reinterpret_cast<const char*>(img) + ((size_t)(((b4 >> 1) * 131 + blockIdx.x * 17) & 63)) * 20480;
        char* dst = smem + 49152 + ((b4 >> 1) & 1) * 21504;
#pragma unroll
        for (int c = 0; c < 6; ++c)
          if (wid + 4 * c < 21) glds16(src + ((wid + 4 * c) % 20) * 1024 + lane * 16, dst + (wid + 4 * c) * 1024);
      }
#pragma unroll
      for (int slot = 0; slot < 14; ++slot) {
        __builtin_amdgcn_sched_barrier(0);
        if (slot == 10 || slot == 12) {
          const int q = (slot - 10) / 2;
          if (q == 0) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(wd16) : "a"(aj[q]), "a"(bi[q]));
          else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(wd16) : "a"(aj[q]), "a"(bi[q]));
        } else {
          const int m = slot < 10 ? slot : (slot == 11 ? 10 : 11);
          // ORDER 0: (k-step, probe block, product) as the library kernel; 1: (probe block, k-step, product): six MFMAs in a row on one accumulator;
          // 2: product-major (hi hi x 4, hi lo x 4, lo hi x 4): the accumulator changes with every MFMA
          const int s = ORDER == 1 ? (m / 3) % 2 : (ORDER == 2 ? (m / 2) % 2 : m / 6), nb = ORDER == 1 ? m / 6 : (ORDER == 2 ? m % 2 : (m / 3) % 2), w = ORDER == 2 ? m / 4 : m % 3;
          const int a = (b & 3) * 2 + nb;
          acc16[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w == 2 ? alc[s] : ahc[s], w == 1 ? vf[s * 4 + nb * 2 + 1] : vf[s * 4 + nb * 2], acc16[a], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (CHAIN) {
          constexpr int e0[16] = {0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13};
          constexpr int h0[8] = {2, 4, 6, 7, 9, 11, 12, 14};
          constexpr int m0[16] = {3, 4, 5, 6, 7, 8, 8, 9, 10, 11, 12, 13, 13, 14, 15, 16};
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (e0[i] % 14 == slot) chain_op(wn, ahn, aln, lp, 0, i);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (h0[i] % 14 == slot) chain_op(wn, ahn, aln, lp, 1, i);
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (m0[i] % 14 == slot) chain_op(wn, ahn, aln, lp, 2, i);
        }
        if ((b & 3) == 3 && slot < 8) vf[slot] = *reinterpret_cast<const half8*>(vb + slot * 1024 + 1024);
        if ((b & 3) == 1 && slot < 2) aj[slot] = *reinterpret_cast<const half8*>(vb + (9 + slot) * 1024);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (DMA && b == 0 && (b4 & 1)) {  // behind block 4 of the tile, as the kernel
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      ahc[0] = ahn[0]; ahc[1] = ahn[1];
      alc[0] = aln[0]; alc[1] = aln[1];
#pragma unroll
      for (int r = 0; r < 16; ++r) wn[r] = wd16[r];
    };
    body(std::integral_constant<int, 0>{});
    body(std::integral_constant<int, 1>{});
    body(std::integral_constant<int, 2>{});
    body(std::integral_constant<int, 3>{});
  }
  const long long t1 = __builtin_readcyclecounter();
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (tid == 0) cyc[blockIdx.x] = t1 - t0;
  float s = 0;
  for (int q = 0; q < 8; ++q)
    for (int r = 0; r < 16; ++r) s += acc16[q][r];
  if (s == 12345.678f) out[0] = s;
}

_Float16* g_img = nullptr;  // 64 tile images of 20 KiB, laid out like the LDS buffers (distance operands small)
template <typename F>
void time_it(const char* name, F launch, int blocks_per_call) {
  long long* cyc;
  hipMalloc(&cyc, 256 * 8);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  launch(cyc, 20);
  float best = 1e30f;
  double cycles = 0;
  for (int it = 0; it < 3; ++it) {
    hipEventRecord(e0);
    launch(cyc, 1);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    long long h[256];
    hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
    double mean = 0;
    for (int i = 0; i < 256; ++i) mean += (double)h[i];
    mean /= 256;
    if (ms < best) { best = ms; cycles = mean; }
  }
  printf("%-58s %7.1f ns per 32x32 block, %7.1f cycles per block, %.2f GHz\n", name, best * 1e6 / blocks_per_call, cycles / blocks_per_call,
         cycles / (best * 1e-3) * 1e-9);
  fflush(stdout);
  hipFree(cyc);
}

template <int VAR>
void run16(const char* name, const _Float16* rnd, float* d) {
  extern _Float16* g_img;
  const int tiles = 50000;  // 8 blocks of 32 x 32 per tile: 400000 blocks, ~0.1 s
  hipFuncSetAttribute(reinterpret_cast<const void*>(k16<VAR>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
  time_it(name, [&](long long* cyc, int div) { k16<VAR><<<256, 256, 40960>>>(rnd, g_img, d, cyc, tiles / div); }, tiles * 8);
}
template <int CHAIN, int ORDER = 0, int DMA = 0>
void run32(const char* name, const _Float16* rnd, float* d) {
  extern _Float16* g_img;
  const int blocks = 400000;
  constexpr int kSmem = DMA ? 49152 + 2 * 21504 : 65536;
  hipFuncSetAttribute(reinterpret_cast<const void*>(k32<CHAIN, ORDER, DMA>), hipFuncAttributeMaxDynamicSharedMemorySize, kSmem);
  time_it(name, [&](long long* cyc, int div) { k32<CHAIN, ORDER, DMA><<<256, 256, kSmem>>>(rnd, g_img, d, cyc, blocks / div); }, blocks);
}

int main() {
  const size_t n = 1 << 21;
  _Float16* h = (_Float16*)malloc(n * 2);
  srand(3);
  for (size_t i = 0; i < n; ++i) h[i] = (_Float16)((rand() % 4001 - 2000) * 4.0f);
  _Float16* rnd;
  hipMalloc(&rnd, n * 2);
  hipMemcpy(rnd, h, n * 2, hipMemcpyHostToDevice);
  float* d;
  hipMalloc(&d, 64);
  {
    const size_t m = 64 * 20480 / 2;
    _Float16* hi = (_Float16*)malloc(m * 2);
    for (size_t i = 0; i < m; ++i) {
      const float v = (rand() % 4001 - 2000) * 4.0f;
      hi[i] = (_Float16)(((i / 512) % 20) >= 16 ? v * (1.f / 12000.f) : v);
    }
    hipMalloc(&g_img, m * 2);
    hipMemcpy(g_img, hi, m * 2, hipMemcpyHostToDevice);
  }
  for (int rep = 0; rep < 2; ++rep) {
    run32<1>("32x32x16 + chain + LDS reads (shape_bench SHAPE 0)", rnd, d);
    run32<1, 0, 1>("32x32x16 + chain + LDS reads + DMA/barrier  [like for like]", rnd, d);
    run32<0>("32x32x16 MFMAs only", rnd, d);
    run32<1, 1>("32x32x16 + chain, six in a row per accumulator", rnd, d);
    run32<1, 2>("32x32x16 + chain, product-major", rnd, d);
    run32<0, 1>("32x32x16 MFMAs only, six in a row", rnd, d);
    run32<0, 2>("32x32x16 MFMAs only, product-major", rnd, d);
    run16<0>("16x16x32 MFMAs only, product-major", rnd, d);
    run16<2>("16x16x32 MFMAs only, accumulator-major", rnd, d);
    run16<1>("16x16x32 + chain T0", rnd, d);
    run16<1 + 32>("16x16x32 + chain T1", rnd, d);
    run16<1 + 2>("16x16x32 + chain T0, accumulator-major", rnd, d);
    run16<1 + 4>("16x16x32 + chain T0 + LDS reads", rnd, d);
    run16<1 + 4 + 8>("16x16x32 + chain T0 + LDS reads + DMA/barrier", rnd, d);
    run16<1 + 4 + 8 + 512>("16x16x32 + chain T0 + reads + DMA/barrier, two tiles/iter", rnd, d);
    run16<1 + 4 + 8 + 32>("16x16x32 + chain T1 + LDS reads + DMA/barrier", rnd, d);
    run16<4 + 8>("16x16x32 MFMAs + LDS reads + DMA/barrier", rnd, d);
    run16<1 + 2 + 128 + 256>("16x16x32 acc-major + exps only", rnd, d);
    run16<1 + 2 + 64 + 256>("16x16x32 acc-major + cvt_pk only", rnd, d);
    run16<1 + 2 + 64 + 128>("16x16x32 acc-major + mixlo/hi only", rnd, d);
    run16<1 + 2 + 256>("16x16x32 acc-major + exps + cvt_pk", rnd, d);
    run16<1 + 2 + 64>("16x16x32 acc-major + cvt_pk + mix", rnd, d);
    run16<2 + 4>("16x16x32 acc-major + LDS reads", rnd, d);
  }
  return 0;
}
