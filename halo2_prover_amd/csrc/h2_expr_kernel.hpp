// h2_expr_kernel.hpp -- an expression DAG compiled to a straight-line program (h2_expr_program.hpp) and the kernel that
// interprets it per row, over any of the three scalar fields.  create_proof's quotient numerator (every gate, the
// permutation argument, the y-fold) is one such program over bn256::Fr; h2_expr_eval_device runs a caller's.
#pragma once
#include <hip/hip_runtime.h>

#include "h2_field.hpp"
#include "h2_field29.hpp"

namespace h2 {
namespace pk {

// operand word: bits 31..30 = kind (0 slot, 1 constant, 2 column, 3 the previous instruction's result); slot / constant:
// index in bits 29..0; column: index in bits 29..8, rotation + 128 in bits 7..0.
// op_dst: op in bits 31..24 (0 add, 1 sub, 2 mul), slot in 23..0 (X_NO_STORE: only the next instruction reads it).
struct XInstr {
  uint32_t op_dst, a, b;
};
constexpr uint32_t X_SLOT = 0u << 30, X_CONST = 1u << 30, X_COL = 2u << 30, X_PREV = 3u << 30;
constexpr uint32_t X_NO_STORE = 0xFFFFFFu;     // destination field of a result that only the next instruction reads
constexpr int EXPR_BLOCK = 64;
constexpr int EXPR_REG_SLOTS = 4;       // slots kept in registers (expr_kernel); the rest is LDS
constexpr size_t EXPR_LDS_MAX = 160 * 1024;   // dynamic LDS one workgroup may hold (expr_kernel has no static LDS)
// magnitudes, in units of p, that the host's compiler (ExprProgramT::compile) assumes: a column operand after
// expr_column_operand, and the largest value an instruction may produce before it is reduced by a product with one
constexpr int EXPR_COLUMN_BOUND = 16, EXPR_VALUE_BOUND = 32;
// what the compiler takes for p / R' when it bounds a product: 2^-7 (1 + 2^-40).  bn256::Fr has p / 2^261 < 0.0059; the
// Pasta primes are 2^254 + t with t < 2^126, so p / 2^261 = 2^-7 (1 + t / 2^254) exceeds 1/128 itself -- by less than
// 2^-127 relative, which the 2^-40 covers together with the roundings of the compiler's double arithmetic (below)
constexpr double EXPR_PRODUCT_SCALE = (1.0 + 0x1p-40) / 128.0;

// The arithmetic runs on the 9 x 29-bit lazy form (h2_field29.hpp: for bn256::Fr a product is ~240 instructions
// against ~600 on 8 x 32-bit limbs with carries):
//   * a column holds x 2^256 (canonical); shifted left by five bits while it is unpacked that is the integer
//     x 2^261 + (a multiple of p) < 32 p, the working form of x -- minus 16 p it lies in [-16 p, 16 p);
//   * the constant table is uploaded in the working form (c 2^261 mod p, canonical) and only unpacked;
//   * sums and differences are carry-normalised, products need nothing; the compiler keeps every value that is stored
//     or forwarded below EXPR_VALUE_BOUND p (it multiplies a sum by one where it would exceed that bound: the sum, at
//     most 2 EXPR_VALUE_BOUND p, is then that product's operand).  fe29_mul needs only its limb bounds, which every
//     normalised value of magnitude below 2^260 meets; a product of two such values, up to (32 p)^2 = 1024 p^2, is
//     past the 64 p^2 that gives fe29_mul's (-3p/2, p/2] range, and lies in (a b / R' - p, a b / R'], |x| < 9 p;
//     fe29_to_api takes any |x| < 64 p;
//   * the last result goes back to the API form (one product) on its way out.
//
// The bounds for every field.  The compiler tracks, per value, a double B with the claim |value| <= B p:
//   constants and variables  canonical in the working form: B = 1, exact;
//   columns                  [-16 p, 16 p): B = 16, exact;
//   a product                |a b| / R' + p <= (Ba Bb (p / R') + 1) p, and the compiler takes
//                            B = Ba Bb EXPR_PRODUCT_SCALE + 1 in doubles;
//   a sum or difference      B = Ba + Bb in doubles; above EXPR_VALUE_BOUND it is reduced by a product with one.
// Doubles round, by at most 2^-53 relative per operation.  Call rho the relative amount by which a value may really
// exceed its B.  Leaves have rho = 0.  A sum has rho <= max(rho_a, rho_b) + 2^-53; every operand of a sum has B >= 1
// and a sum above 32 is reduced, so a tree of sums that no product interrupts is at most 64 deep: rho <= 2^-47 there.
// A product really is at most Ba (1 + rho_a) Bb (1 + rho_b) (p / R') + 1 <= Ba Bb 2^-7 (1 + 2^-46 + 2^-127) + 1, and the
// computed B is at least Ba Bb 2^-7 (1 + 2^-40) (1 - 2^-51) + 1, which is larger: a product has rho = 0 again, for
// bn256::Fr and for the Pasta primes alike.  So every value the kernel keeps or forwards is at most 32 p (1 + 2^-47) and
// a sum before its reduction at most 64 p (1 + 2^-47).  With p < 2^254 (1 + 2^-126) that is below 2^260 (1 + 2^-46): the
// top limb of the normalised form (the value >> 232) has magnitude at most 2^28 + 1, the others lie in [0, 2^29) --
// fe29_mul's limb bounds hold on either side with a factor of two to spare; two such limb vectors add within int32
// before fe29_norm; and the root, a kept value, is far inside fe29_to_api's |x| < 64 p.  Concrete rows cannot even
// reach the 2^-47: the only values that sit exactly on a bound are sums of columns at -16 p, and those are exact in
// doubles (tests/test_expr_public.py asserts 32 p and 64 p themselves on every row, for the three fields).
//
// Operands that do not depend on the program's own results -- columns and constants -- are fetched TWO instructions
// ahead (a global load is 0.5-2 us, an instruction 0.1-0.5).  LDS: 36 bytes per slot beyond the register slots and row.
// grid.y = instance (a proof of create_proofs, an instance of h2_expr_eval_device).  One program and one set of row
// masks; instance p reads its column pointers at all_cols + p ncols, its constants (the variables differ: y, beta,
// gamma, beta delta^j) at all_consts + p nconsts and writes rows [0, en) of the column all_out + p out_stride.
// Every index is formed from the row, the instruction words (constant, column and slot numbers proven against the
// table sizes when the program was compiled) and col_mask: a column element that is not canonical changes the value,
// never an address.
template <class FP>
static __global__ void __launch_bounds__(EXPR_BLOCK)
expr_kernel(const XInstr* __restrict__ prog, uint32_t ninstr, const U128* const* __restrict__ all_cols, uint32_t ncols,
            const uint32_t* __restrict__ col_mask, const U128* __restrict__ all_consts, uint32_t nconsts,
            U128* __restrict__ all_out, size_t out_stride, uint32_t step, uint32_t en) {
  const U128* const* __restrict__ cols = all_cols + (size_t)blockIdx.y * ncols;
  const U128* __restrict__ consts = all_consts + 2 * (size_t)blockIdx.y * nconsts;
  U128* __restrict__ out = all_out + 2 * (size_t)blockIdx.y * out_stride;
  using F = Fe<FP>;
  using W = Fe29<FP>;
  extern __shared__ int32_t slots[];      // [slot][limb][thread]
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x * EXPR_BLOCK + tid;
  // slots 0 .. EXPR_REG_SLOTS-1 live in registers: the slot number comes from the instruction word, the same for the
  // whole wave, so the choice is a scalar branch around nine moves -- nothing next to a 240-instruction product, and
  // the LDS that is left (Poseidon: 3 slots instead of 7) no longer caps the waves per SIMD
  W reg0 = W::zero(), reg1 = W::zero(), reg2 = W::zero(), reg3 = W::zero();
  auto slot_load = [&](uint32_t s) {
    if (s == 0) return reg0;
    if (s == 1) return reg1;
    if (s == 2) return reg2;
    if (s == 3) return reg3;
    W r;
#pragma unroll
    for (int l = 0; l < 9; l++) r.v[l] = slots[((s - EXPR_REG_SLOTS) * 9 + l) * EXPR_BLOCK + tid];
    return r;
  };
  // a column or constant operand as loaded (a slot operand is read when its instruction runs)
  auto fetch = [&](uint32_t code) -> F {
    const uint32_t kind = code & (3u << 30);
    if (kind == X_SLOT || kind == X_PREV) return F::zero();
    if (kind == X_CONST) return fe_load<FP>(consts + 2 * (size_t)(code & 0x3FFFFFFFu));
    const uint32_t c = (code >> 8) & 0x3FFFFFu;
    const int rot = (int)(code & 0xFFu) - 128;
    const uint32_t idx = (i + (uint32_t)(rot * (int)step)) & col_mask[c];
    return fe_load<FP>(cols[c] + 2 * (size_t)idx);
  };
  const XInstr nop{0u, X_SLOT, X_SLOT};
  auto instr_at = [&](uint32_t k) { return k < ninstr ? prog[k] : nop; };
  W r = W::zero();
  auto operand = [&](uint32_t code, const F& pre) -> W {
    const uint32_t kind = code & (3u << 30);
    if (kind == X_SLOT) return slot_load(code & 0x3FFFFFFFu);
    if (kind == X_PREV) return r;
    if (kind == X_CONST) return fe29_unpack(pre);
    return expr_column_operand(pre);
  };
  // one instruction: operands from the prefetched pair, the register or LDS; the pair is refilled for instruction k + 2
  // (the instruction words travel the same way: `ins` was read two instructions ago and is replaced by the one two ahead)
  auto run = [&](uint32_t k, XInstr& slot_ins, F& pa, F& pb) {
    const XInstr ins = slot_ins;
    const W a = operand(ins.a, pa), b = operand(ins.b, pb);
    const XInstr ahead = instr_at(k + 2);
    slot_ins = ahead;
    pa = fetch(ahead.a);
    pb = fetch(ahead.b);
    const uint32_t op = ins.op_dst >> 24;
    if (op == 2) r = fe29_mul(a, b);
    else r = fe29_norm(op == 0 ? fe29_add(a, b) : fe29_sub(a, b));
    const uint32_t s = ins.op_dst & 0xFFFFFFu;
    if (s == 0) reg0 = r;
    else if (s == 1) reg1 = r;
    else if (s == 2) reg2 = r;
    else if (s == 3) reg3 = r;
    else if (s != X_NO_STORE) {
#pragma unroll
      for (int l = 0; l < 9; l++) slots[((s - EXPR_REG_SLOTS) * 9 + l) * EXPR_BLOCK + tid] = r.v[l];
    }
  };
  XInstr i0 = instr_at(0), i1 = instr_at(1);
  F pa0 = fetch(i0.a), pb0 = fetch(i0.b), pa1 = fetch(i1.a), pb1 = fetch(i1.b);
  for (uint32_t k = 0; k < ninstr; k += 2) {
    run(k, i0, pa0, pb0);
    if (k + 1 < ninstr) run(k + 1, i1, pa1, pb1);
  }
  if (i < en) fe_store<FP>(out + 2 * (size_t)i, fe29_to_api(r));     // a domain smaller than one block: the spare lanes computed on wrapped rows
}

// LDS of a program with `nslots` live-value slots: the slots beyond the registers, nine limbs of EXPR_BLOCK rows each
// (may exceed EXPR_LDS_MAX: the caller refuses such a program)
inline size_t expr_lds_for_slots(uint32_t nslots) {
  const size_t lds_slots = nslots > (uint32_t)EXPR_REG_SLOTS ? nslots - EXPR_REG_SLOTS : 1;
  return lds_slots * 9 * EXPR_BLOCK * 4;
}

// expr_kernel over `en` rows of 1 <= count <= 65535 instances (grid.y); lds <= EXPR_LDS_MAX as expr_lds_for_slots gave it
template <class FP>
hipError_t expr_kernel_launch(const XInstr* d_code, uint32_t ninstr, const U128* const* d_ptrs, uint32_t ncols, const uint32_t* d_masks,
                              const U128* d_consts, uint32_t nconsts, U128* d_out, size_t out_stride, uint32_t step, uint32_t en,
                              uint32_t count, size_t lds, hipStream_t s) {
  if (count == 0 || count > 65535 || lds > EXPR_LDS_MAX || ninstr == 0) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {                              // past 64 KiB: raised, as the MSM and NTT kernels raise theirs
    const hipError_t e = hipFuncSetAttribute((const void*)expr_kernel<FP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(expr_kernel<FP>, dim3((en + EXPR_BLOCK - 1) / EXPR_BLOCK, count), dim3(EXPR_BLOCK), lds, s, d_code, ninstr, d_ptrs,
                     ncols, d_masks, d_consts, nconsts, d_out, out_stride, step, en);
  return hipGetLastError();
}

}  // namespace pk
}  // namespace h2
