// Shared LDS-tile helpers for the flash attention forward/backward kernels
// (gfx950). Row-major 64-row x D-col bf16 tiles at a fixed 256 B row stride
// with the T2 XOR swizzle; MFMA fragment production via hardware transpose
// reads and in-register cvt_pk+permlane transforms.
#pragma once

#include "common.h"

#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) int i32x2;

// The counted lgkmcnt(N) waits in tr_quad_wait/tr_pair_wait assume (a) DS
// ops complete in order and (b) the compiler schedules no lgkm-counted op
// of its own between issue and wait. (b) is verified against the toolchains
// we have measured; a new major compiler version must be re-validated with
// the GPU parity tests (tests/test_gpu_ops.py) before this guard is
// extended. ZTA_SAFE_WAITS=1 turns every counted wait into lgkmcnt(0) to
// bisect silent corruption if scheduling ever changes.
#if defined(__HIP_DEVICE_COMPILE__) && defined(__clang_major__)
#if __clang_major__ < 19 || __clang_major__ > 22
#error \
    "attn_tiles.h counted s_waitcnt contracts validated only for ROCm LLVM 19-22; \
re-run tests/test_gpu_ops.py on this compiler and extend the guard (or build \
with -DZTA_SAFE_WAITS=1)."
#endif
#endif
#ifndef ZTA_SAFE_WAITS
#define ZTA_SAFE_WAITS 0
#endif

namespace attn {

constexpr int NW = 8;        // waves per block
constexpr int RB = NW * 32;  // rows (q or kv) owned per block
constexpr int TB = 64;       // staged tile rows per iteration

ZTA_DEV int swz(int row, int byte_off) { return byte_off ^ ((row & 7) << 4); }

// Row of a 32x32 MFMA C/D tile held by accumulator register r of a lane in
// half hi = lane >> 5 (the column is lane & 31).
ZTA_DEV constexpr int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// Element offsets of the planes of one (b, h) = (bh / H, bh % H) in the
// packed tensors: q, k and v columns of qkv / dqkv (B, T, 3C), row stride
// QS = 3C, and the same head's columns of a (B, T, C) tensor (o, dout), row
// stride C. Head dim D = C / H.
struct Planes {
  int h, QS;
  long base, kbase, vbase, obase;
};
template <int D>
ZTA_DEV Planes planes(int bh, int H, int T, int C) {
  const int h = bh % H;
  const int QS = 3 * C;
  const long base = (long)(bh / H) * T * QS + h * D;
  return {h, QS, base, base + C, base + 2 * C, (long)(bh / H) * T * C + h * D};
}

// Dropout of the counter RNG (common.h drop_bits32): a key is kept iff its
// hash byte >= thr = round(256 p); kept values scale by 256 / (256 - thr).
// Forward and backward must agree on both, so they are defined once.
__host__ ZTA_DEV uint32_t drop_thr(float p_drop) { return (uint32_t)(p_drop * 256.0f + 0.5f); }
ZTA_DEV float drop_inv_keep(uint32_t thr) { return thr ? 256.0f / (256.0f - (float)thr) : 1.0f; }

// B-fragments of mfma_f32_32x32x16_bf16 via hardware transpose reads: lane l
// receives tile[k0 + 8*(l>>5) + e][j0 + (l&31)] for e = 0..7 from a
// row-major bf16 LDS tile with 256 B row stride and the T2 XOR swizzle.
//
// ds_read_b64_tr_b16 semantics (measured, tools/probes/tr_probe.hip): within
// each 16-lane group, out[lane 4a+b][reg j] = in[lane 4j+a][elem b] — i.e.
// lane l supplies row ((l>>2)&3), column-block 4*(l&3) of a [4][16] tile and
// receives the column (l%16) of that tile, rows ascending over the 4 regs.
// Ordering contract for the transpose-read asms below:
//  * a read and its wait must be tied together: SIInsertWaitcnts cannot see
//    a ds_read inside inline asm, so it inserts no lgkmcnt wait before uses
//    of its outputs, and a bare waitcnt asm has no dataflow edge to the
//    outputs — the scheduler may move the consuming MFMA between read and
//    wait (observed: register-junk O values with exact lse). Either both sit
//    in ONE asm statement, or — the pipelined issue/wait pairs below — the
//    wait statement takes the fragment registers as "+v" pass-through
//    operands, so that every consumer depends on it.
//  * "=&v" (early clobber) keeps a read's destination from aliasing an
//    address operand that a later read of the same statement still needs.
//  * the asms carry NO "memory" clobber — a clobber on every fragment read
//    made each one a full scheduling barrier and serialized the whole MFMA
//    accumulation loop. Instead the kernel calls lds_acquire() ONCE after
//    the tile-ready __syncthreads(): volatile asms are not reordered with
//    respect to each other, so the clobbered empty asm (a) keeps the
//    staging stores alive (a may-read-everything point after them) and
//    (b) pins every later volatile tr-read below the barrier.
ZTA_DEV void lds_acquire() { asm volatile("" ::: "memory"); }

// Two B-fragments (k0..k0+15 and k0+16..k0+31): four transpose reads.
struct TrPair {
  bf16x8 a, b;
};
// Pairs from TWO tiles (same k0/j0): eight transpose reads in one asm — for
// the dKdV loop, which needs dO^T and Q^T fragments per d.
struct TrQuad {
  TrPair x, y;
};

// Software-pipelined transpose reads: tr_quad_issue launches the eight
// reads with NO wait; tr_quad_wait waits `lgkmcnt(N)` with the fragment
// registers as pass-through operands so every consumer orders after it.
// Safety: DS ops complete IN ORDER, so waiting with N = (number of DS ops
// issued after this group) is correct even if the compiler interleaves its
// own LDS ops — any overcount only waits longer. (SMEM also counts in
// lgkmcnt and completes out of order, but none is live in these loops.)
// `l` is the lane id; a kernel whose tile loop must not carry hoisted
// per-lane addresses (register pressure) passes a loop-local opaque copy.
ZTA_DEV void tr_quad_issue(const uint16_t* lds_x, const uint16_t* lds_y, int k0,
                           int j0, TrQuad* out, int l = threadIdx.x & 63) {
  const int colb = (j0 + (l & 16) + 4 * (l & 3)) * 2;
  const int rb = 8 * (l >> 5) + ((l >> 2) & 3);
  int ax[4], ay[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = k0 + 16 * (i >> 1) + 4 * (i & 1) + rb;
    const int off = row * 256 + (colb ^ ((row & 7) << 4));
    ax[i] = (int)(size_t)((const char*)lds_x + off);
    ay[i] = (int)(size_t)((const char*)lds_y + off);
  }
  union U {
    i32x2 d[8];
    TrQuad f;
  }* u = (union U*)out;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %9\n\t"
      "ds_read_b64_tr_b16 %2, %10\n\t"
      "ds_read_b64_tr_b16 %3, %11\n\t"
      "ds_read_b64_tr_b16 %4, %12\n\t"
      "ds_read_b64_tr_b16 %5, %13\n\t"
      "ds_read_b64_tr_b16 %6, %14\n\t"
      "ds_read_b64_tr_b16 %7, %15"
      : "=&v"(u->d[0]), "=&v"(u->d[1]), "=&v"(u->d[2]), "=&v"(u->d[3]),
        "=&v"(u->d[4]), "=&v"(u->d[5]), "=&v"(u->d[6]), "=&v"(u->d[7])
      : "v"(ax[0]), "v"(ax[1]), "v"(ax[2]), "v"(ax[3]), "v"(ay[0]), "v"(ay[1]),
        "v"(ay[2]), "v"(ay[3]));
}

// Quad for the fused backward's dQ = dS K product (same issue / counted-wait
// contract as tr_quad_issue, drained with tr_quad_wait): x is the A-fragment
// pair of dS, transpose-read from the workgroup's bf16 dS tile
// [key][32 q rows] (64 B rows, unswizzled — lane l receives
// tile[k0 + 8*(l>>5) + e][l&31], i.e. A[i = q][k = key]); y is the
// B-fragment pair of K, columns j0..j0+31, from the swizzled 256 B-row K
// image. Keys k0..k0+15 land in .a, k0+16..k0+31 in .b.
ZTA_DEV void tr_dsk_issue(const uint16_t* ds_tile, const uint16_t* k_img, int k0,
                          int j0, TrQuad* out, int l = threadIdx.x & 63) {
  const int cq = ((l & 16) + 4 * (l & 3)) * 2;
  const int colb = (j0 + (l & 16) + 4 * (l & 3)) * 2;
  const int rb = 8 * (l >> 5) + ((l >> 2) & 3);
  int ax[4], ay[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = k0 + 16 * (i >> 1) + 4 * (i & 1) + rb;
    ax[i] = (int)(size_t)((const char*)ds_tile + row * 64 + cq);
    ay[i] = (int)(size_t)((const char*)k_img + row * 256 + (colb ^ ((row & 7) << 4)));
  }
  union U {
    i32x2 d[8];
    TrQuad f;
  }* u = (union U*)out;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %9\n\t"
      "ds_read_b64_tr_b16 %2, %10\n\t"
      "ds_read_b64_tr_b16 %3, %11\n\t"
      "ds_read_b64_tr_b16 %4, %12\n\t"
      "ds_read_b64_tr_b16 %5, %13\n\t"
      "ds_read_b64_tr_b16 %6, %14\n\t"
      "ds_read_b64_tr_b16 %7, %15"
      : "=&v"(u->d[0]), "=&v"(u->d[1]), "=&v"(u->d[2]), "=&v"(u->d[3]),
        "=&v"(u->d[4]), "=&v"(u->d[5]), "=&v"(u->d[6]), "=&v"(u->d[7])
      : "v"(ax[0]), "v"(ax[1]), "v"(ax[2]), "v"(ax[3]), "v"(ay[0]), "v"(ay[1]),
        "v"(ay[2]), "v"(ay[3]));
}

// Workgroup barrier that also waits this wave's vector-memory operations
// down to the N youngest (vmcnt retires in issue order; LDS-DMA loads, plain
// loads, stores and no-return atomics all count): the wave's LDS-DMA tile
// lands while N later atomics stay in flight. N must not exceed the number
// of vector-memory instructions the wave issued after the DMA group.
template <int N>
ZTA_DEV void tile_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier"
               :
               : "i"(ZTA_SAFE_WAITS ? 0 : N)
               : "memory");
}

// MFMA chains with arch-VGPR accumulators, for kernels whose resident
// accumulators already fill the accumulation-register file: the compiler
// gives every builtin MFMA an AGPR destination, so a transient S / dP / dQ
// tile issued through the builtin would evict resident tiles around each
// use. Hazards the compiler cannot pad inside an asm statement are padded
// here: `s_nop 1` covers a just-written operand, the closing `s_nop 11` the
// 8-pass result -> any reader (each statement may be followed by compiler
// copies of the accumulator). Accumulate chains need no pad in between.
//
// Two k-steps of S += A_q B_k and dP += A_do B_v (C[i=q][j=key]); FIRST
// starts both chains from zero.
template <bool FIRST>
ZTA_DEV void mfma_sdp2(f32x16& s, f32x16& dp, const bf16x8* qa, const bf16x8* da,
                       const bf16x8* kb, const bf16x8* vb) {
  if (FIRST) {
    asm("s_nop 1\n\t"
        "v_mfma_f32_32x32x16_bf16 %0, %2, %6, 0\n\t"
        "v_mfma_f32_32x32x16_bf16 %1, %4, %8, 0\n\t"
        "v_mfma_f32_32x32x16_bf16 %0, %3, %7, %0\n\t"
        "v_mfma_f32_32x32x16_bf16 %1, %5, %9, %1\n\t"
        "s_nop 11"
        : "=&v"(s), "=&v"(dp)
        : "v"(qa[0]), "v"(qa[1]), "v"(da[0]), "v"(da[1]), "v"(kb[0]), "v"(kb[1]),
          "v"(vb[0]), "v"(vb[1]));
  } else {
    asm("s_nop 1\n\t"
        "v_mfma_f32_32x32x16_bf16 %0, %2, %6, %0\n\t"
        "v_mfma_f32_32x32x16_bf16 %1, %4, %8, %1\n\t"
        "v_mfma_f32_32x32x16_bf16 %0, %3, %7, %0\n\t"
        "v_mfma_f32_32x32x16_bf16 %1, %5, %9, %1\n\t"
        "s_nop 11"
        : "+v"(s), "+v"(dp)
        : "v"(qa[0]), "v"(qa[1]), "v"(da[0]), "v"(da[1]), "v"(kb[0]), "v"(kb[1]),
          "v"(vb[0]), "v"(vb[1]));
  }
}

// acc += x.a y.a + x.b y.b for a quad already drained with tr_quad_wait.
ZTA_DEV void mfma_quad_acc(f32x16& acc, const TrQuad& t) {
  asm("s_nop 1\n\t"
      "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\t"
      "v_mfma_f32_32x32x16_bf16 %0, %3, %4, %0\n\t"
      "s_nop 11"
      : "+v"(acc)
      : "v"(t.x.a), "v"(t.y.a), "v"(t.x.b), "v"(t.y.b));
}

// Workgroup barrier that orders LDS traffic only: drains this wave's DS ops
// (lgkmcnt) but NOT vmcnt, so global atomics issued before it stay in
// flight. The "memory" clobber keeps plain LDS stores above it and, being a
// volatile asm, every later transpose read stays below it.
ZTA_DEV void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int N>
ZTA_DEV void tr_quad_wait(TrQuad* q) {
  union U {
    i32x2 d[8];
    TrQuad f;
  }* u = (union U*)q;
  asm volatile("s_waitcnt lgkmcnt(%8)"
               : "+v"(u->d[0]), "+v"(u->d[1]), "+v"(u->d[2]), "+v"(u->d[3]),
                 "+v"(u->d[4]), "+v"(u->d[5]), "+v"(u->d[6]), "+v"(u->d[7])
               : "i"(ZTA_SAFE_WAITS ? 0 : N));
}

// Pipelined pair form (see tr_quad_issue/tr_quad_wait for the contract).
ZTA_DEV void tr_pair_issue(const uint16_t* lds, int k0, int j0, TrPair* out) {
  const int l = threadIdx.x & 63;
  const int colb = (j0 + (l & 16) + 4 * (l & 3)) * 2;
  const int rb = 8 * (l >> 5) + ((l >> 2) & 3);
  int a[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = k0 + 16 * (i >> 1) + 4 * (i & 1) + rb;
    a[i] = (int)(size_t)((const char*)lds + row * 256 + (colb ^ ((row & 7) << 4)));
  }
  union U {
    i32x2 d[4];
    TrPair f;
  }* u = (union U*)out;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %6\n\t"
      "ds_read_b64_tr_b16 %3, %7"
      : "=&v"(u->d[0]), "=&v"(u->d[1]), "=&v"(u->d[2]), "=&v"(u->d[3])
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));
}

// Base + immediate form of tr_pair_issue. For k0 a multiple of 8 and j0 a
// multiple of 32 the swizzled address of tr_pair_issue splits into a
// lane-constant term and a compile-time term (the XOR touches bits 4-5 from
// the lane and bit 6 from the read index only), so the four reads share ONE
// address register and carry their row / d-block in the DS offset field:
//   addr = lds + tr_lane_off(l) + (K0 + 16*(i>>1) + 4*(i&1))*256
//              + ((2*J0) ^ ((i&1) << 6)).
ZTA_DEV int tr_lane_off(int l) {
  const int q = (l >> 2) & 3;
  return (8 * (l >> 5) + q) * 256 + ((2 * (l & 16) + 8 * (l & 3)) ^ (q << 4));
}
template <int K0, int J0>
ZTA_DEV void tr_pair_issue_imm(int lane_base, TrPair* out) {
  static_assert(K0 % 8 == 0 && J0 % 32 == 0, "offset split needs aligned k0/j0");
  constexpr int O0 = (K0 + 0) * 256 + (2 * J0);
  constexpr int O1 = (K0 + 4) * 256 + ((2 * J0) ^ 64);
  constexpr int O2 = (K0 + 16) * 256 + (2 * J0);
  constexpr int O3 = (K0 + 20) * 256 + ((2 * J0) ^ 64);
  union U {
    i32x2 d[4];
    TrPair f;
  }* u = (union U*)out;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4 offset:%5\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:%6\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:%7\n\t"
      "ds_read_b64_tr_b16 %3, %4 offset:%8"
      : "=&v"(u->d[0]), "=&v"(u->d[1]), "=&v"(u->d[2]), "=&v"(u->d[3])
      : "v"(lane_base), "n"(O0), "n"(O1), "n"(O2), "n"(O3));
}

template <int N>
ZTA_DEV void tr_pair_wait(TrPair* q) {
  union U {
    i32x2 d[4];
    TrPair f;
  }* u = (union U*)q;
  asm volatile("s_waitcnt lgkmcnt(%4)"
               : "+v"(u->d[0]), "+v"(u->d[1]), "+v"(u->d[2]), "+v"(u->d[3])
               : "i"(ZTA_SAFE_WAITS ? 0 : N));
}

// In-register C-layout -> A-fragment transform (T12): 16 f32 values x[r]
// laid out C[i = crow(r,hi)][j = lane&31] become two bf16x8 A-fragments
// pa[s2] with lane l holding A[i = l&31][k = s2*16 + 8*(l>>5) + e].
ZTA_DEV void c_to_a_frags(const float* x, bf16x8* pa) {
  unsigned w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w[j]) : "v"(x[2 * j]), "v"(x[2 * j + 1]));
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    auto r0 = __builtin_amdgcn_permlane32_swap(w[4 * j + 0], w[4 * j + 2], false, false);
    w[4 * j + 0] = r0[0];
    w[4 * j + 2] = r0[1];
    auto r1 = __builtin_amdgcn_permlane32_swap(w[4 * j + 1], w[4 * j + 3], false, false);
    w[4 * j + 1] = r1[0];
    w[4 * j + 3] = r1[1];
  }
  union {
    unsigned u[4];
    bf16x8 v8;
  } cvt;
  cvt.u[0] = w[0]; cvt.u[1] = w[1]; cvt.u[2] = w[2]; cvt.u[3] = w[3];
  pa[0] = cvt.v8;
  cvt.u[0] = w[4]; cvt.u[1] = w[5]; cvt.u[2] = w[6]; cvt.u[3] = w[7];
  pa[1] = cvt.v8;
}

// Direct LDS-DMA staging (global_load_lds_dwordx4) of a 64-row x D-col bf16
// tile into the 256 B-stride XOR-swizzled image: no staging registers, no
// ds_write phase, and (with double-buffered LDS) ONE barrier per tile.
// Semantics measured by tools/probes/glds_probe.hip: the LDS base is
// wave-uniform and lane l's 16 bytes land at base + 16*l, so one
// wave-instruction fills 1 KiB = four 256 B image rows; the per-lane SOURCE
// address carries the swizzle (dest slot s of row r holds source columns
// 8*(s ^ (r&7))..+7 — T2 note: with lane-linear destinations the XOR moves
// to the source side). Rows beyond T are clamped to row T-1: the data is
// finite real-tensor content and every consumer masks those rows to p = 0.
// NWAVES = threads/64; chunk k (4 rows) is staged by wave k % NWAVES.
// ROWS (multiple of 4) stages a shorter tile, e.g. one 32-row slice.
template <int D, int NWAVES, int ROWS = TB>
ZTA_DEV void glds_stage(const uint16_t* g, long base, int rs, int row0, int T,
                        uint16_t* lds, int l = threadIdx.x & 63) {
  const int wave = (threadIdx.x >> 6);
  const int s = l & 15;        // 16 B slot within the 256 B image row
  const int rsub = l >> 4;     // row within the chunk's 4 rows
#pragma unroll
  for (int k = wave; k < ROWS / 4; k += NWAVES) {
    const int row = 4 * k + rsub;
    int c8 = 8 * (s ^ (row & 7));  // swizzled source column block
    if (D < 128 && c8 >= D) c8 = 0;  // slot never read for cols >= D
    const int rg = min(row0 + row, T - 1);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)&g[base + (long)rg * rs + c8],
        (__attribute__((address_space(3))) void*)(lds + (long)k * 512), 16, 0, 0);
  }
}

// LDS-DMA of the per-row f32 statistics of a 32-row slice, one wave
// instruction (4 B per lane): dst[0..31] = a[rowbase + q], dst[32..63] =
// b[rowbase + q] for q = q0..q0+31, rows past T clamped to T-1.
ZTA_DEV void glds_stats32(const float* a, const float* b, long rowbase, int q0, int T,
                          float* dst, int l = threadIdx.x & 63) {
  const float* src = (l < 32 ? a : b) + rowbase + min(q0 + (l & 31), T - 1);
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
}

// Host: f(std::integral_constant<int, D>{}) for a head dim the flash kernels
// are instantiated for; false (f not called) for any other.
template <class F>
bool with_head_dim(int D, F&& f) {
  switch (D) {
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    case 96: f(std::integral_constant<int, 96>{}); return true;
    case 128: f(std::integral_constant<int, 128>{}); return true;
  }
  return false;
}

}  // namespace attn
