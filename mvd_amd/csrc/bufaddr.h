// Buffer addressing of the gfx950 kernels: resource descriptors, LDS-DMA loads and the 16-byte store -- defined once
// (gemm_pp.hip, gemm_sm.hip, gemm_xs.hip, conv_ws.hip, norm.hip, attention.hip and the probe sources).
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void lds_void;

constexpr unsigned OOB = 0x80000000u;   // voffset of a load that must return zeros / a store that is dropped (>= num_records)

// raw buffer descriptor over [p, p + bytes): stride 0, bounds-checked against `bytes`; word 3 = 32-bit data format, which is
// all gfx950 needs for raw (untyped) buffer instructions
// (a macro: through an inlined function the compiler schedules several kernels differently)
#define buf_rsrc(p, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(p), 0, (bytes), 0x00020000)

// one 16-byte-per-lane (dma4: 4-byte-per-lane) LDS-DMA: LDS destination = wave-uniform base + lane * 16 (* 4)
MVD_DEVINL void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_wave_base, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_wave_base, 16, (int)voff, (int)soff, 0, 0);
}
MVD_DEVINL void dma4(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_wave_base, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_wave_base, 4, (int)voff, (int)soff, 0, 0);
}

// 16-byte buffer store + the wait states hipcc does not insert (invariant I5 of DESIGN.md section 0, checked on the compiler's
// output by tools/lint_device_isa.py).  A store of more than 64 bits reads its data registers over several cycles;
// overwriting them in the next instruction corrupts the last lanes' data.  hipcc's hazard recognizer skips this case
// whenever the store's soffset is an SGPR -- as it always is here -- which the older ISAs allowed; on gfx950 it is not
// safe: in the LayerNorm-fold epilogue a v_pk_mul_f32 directly behind a buffer_store_dwordx4 replaced bf16 pairs of lanes
// 12..15 / 28..31 / ... by halves of the fp32 product (NaNs in the output).  The asm READS the data registers, so whatever
// overwrites them is ordered behind the two wait states.
// AUX = cache policy.  0, the default: with the non-temporal hint (aux = 2) the L2 stops merging the four waves' 160-byte row
// pieces into whole lines -- dense class 10.1 -> 12.2 ms/step, fused-LayerNorm 3.4 -> 5.5, 460 -> 425 fwd/s on the same box.
// 16 = sc1, write-through: the split-K partials of gemm_sm.hip, which other workgroups read.
template <int AUX = 0> MVD_DEVINL void store16(u32x4 v, __amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voff, soff, AUX);
  asm volatile("s_nop 1" :: "v"(v));
}
