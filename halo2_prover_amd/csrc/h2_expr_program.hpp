// h2_expr_program.hpp -- the quotient numerator as a straight-line program: the compiler (host) and the launch of the
// kernel that interprets it (h2_prover_kernels.hpp, expr_kernel).
#pragma once
#include <functional>
#include <tuple>

#include "h2_product_dev.hpp"

namespace h2 {
namespace product {

// ---- the quotient numerator compiled to a straight-line program (h2_prover_kernels.hpp expr_kernel) ------------------------
struct ExprProgram {
  // nodes (hash-consed): 0 const, 1 column, 2 add, 3 sub, 4 mul
  struct Node {
    int op, a, b, col, rot, cidx;
    bool operator<(const Node& o) const {
      return std::tie(op, a, b, col, rot, cidx) < std::tie(o.op, o.a, o.b, o.col, o.rot, o.cidx);
    }
  };
  std::vector<Node> nodes;
  std::map<Node, int> index;
  std::vector<Fr> consts;              // constant table (proof-dependent entries are patched per proof)
  std::map<std::array<uint8_t, 32>, int> const_index;
  int intern(const Node& nd) {
    auto it = index.find(nd);
    if (it != index.end()) return it->second;
    nodes.push_back(nd);
    index[nd] = (int)nodes.size() - 1;
    return (int)nodes.size() - 1;
  }
  int constant(const Fr& v) {
    std::array<uint8_t, 32> key;
    memcpy(key.data(), v.v.v, 32);
    auto it = const_index.find(key);
    int ci;
    if (it == const_index.end()) {
      consts.push_back(v);
      ci = (int)consts.size() - 1;
      const_index[key] = ci;
    } else {
      ci = it->second;
    }
    return intern({0, -1, -1, -1, 0, ci});
  }
  // a slot of the constant table whose value is set later (challenges): never merged with another constant
  int variable(int* slot_out) {
    consts.push_back(Fr::zero());
    *slot_out = (int)consts.size() - 1;
    return intern({0, -1, -1, -1, 0, *slot_out});
  }
  int column(int col, int rot) { return intern({1, -1, -1, col, rot, -1}); }
  int add(int a, int b) { return intern({2, std::min(a, b), std::max(a, b), -1, 0, -1}); }
  int sub(int a, int b) { return intern({3, a, b, -1, 0, -1}); }
  int mul(int a, int b) { return intern({4, std::min(a, b), std::max(a, b), -1, 0, -1}); }

  std::vector<pk::XInstr> code;
  uint32_t nslots = 0, nreduce = 0;      // LDS slots; products with one inserted to keep magnitudes bounded
  // emit instructions for `root` (every arithmetic node it depends on, in order), slots reused after the last use.
  // Order: depth first, the operand that needs more live values first (Sethi-Ullman numbering; shared nodes count as
  // computed).  A result that the NEXT instruction consumes is handed over in a register (operand kind X_PREV), and a
  // result with no other use is never stored: a slot costs 32 bytes of LDS per row and the slots of 128 rows decide
  // how many blocks share a CU (h2_prover_kernels.hpp, expr_kernel).
  void compile(int root) {
    for (const Node& nd : nodes)                     // the operand word has 22 bits for a column and 8 for rot + 128
      if (nd.op == 1 && (nd.col < 0 || nd.col >= (1 << 22) || nd.rot < -128 || nd.rot > 127))
        fail(H2_EINVAL, "quotient program: column index or rotation does not fit its operand word");
    (void)constant(Fr::one());                       // the reducing product's operand: interned before the node tables are sized
    std::vector<int> need(nodes.size(), -1);
    std::function<int(int)> su = [&](int id) -> int {
      if (need[id] >= 0) return need[id];
      const Node& nd = nodes[id];
      if (nd.op < 2) return need[id] = 0;
      const int na = su(nd.a), nb = su(nd.b);
      return need[id] = std::max(1, na == nb ? na + 1 : std::max(na, nb));
    };
    su(root);
    std::vector<int> order;
    std::vector<char> seen(nodes.size(), 0);
    std::function<void(int)> visit = [&](int id) {
      if (seen[id]) return;
      seen[id] = 1;
      const Node& nd = nodes[id];
      if (nd.op >= 2) {
        if (need[nd.b] > need[nd.a]) {
          visit(nd.b);
          visit(nd.a);
        } else {
          visit(nd.a);
          visit(nd.b);
        }
        order.push_back(id);
      }
    };
    visit(root);
    if (order.empty()) fail(H2_EINVAL, "empty quotient program");
    std::vector<int> at(nodes.size(), -1);           // instruction index of a node
    for (size_t t = 0; t < order.size(); t++) at[order[t]] = (int)t;
    std::vector<int> last_use(nodes.size(), -1);
    std::vector<char> wants_slot(nodes.size(), 0);   // some use is not the very next instruction
    for (size_t t = 0; t < order.size(); t++)
      for (int src : {nodes[order[t]].a, nodes[order[t]].b}) {
        last_use[src] = (int)t;
        if (nodes[src].op >= 2 && at[src] + 1 != (int)t) wants_slot[src] = 1;
      }
    std::vector<int> slot_of(nodes.size(), -1);
    std::vector<uint32_t> free_slots;
    // magnitudes in units of p (expr_kernel's header): constants are canonical, columns below EXPR_COLUMN_BOUND, a
    // product of a and b below a b / 128 + 1 (p^2 / 2^261 < p / 128); a sum that would pass EXPR_VALUE_BOUND is
    // multiplied by one straight away
    std::vector<double> bound(nodes.size(), 0.0);
    for (size_t id = 0; id < nodes.size(); id++)
      if (nodes[id].op == 0) bound[id] = 1.0;
      else if (nodes[id].op == 1) bound[id] = pk::EXPR_COLUMN_BOUND;
    const uint32_t one_operand = pk::X_CONST | (uint32_t)nodes[constant(Fr::one())].cidx;
    for (size_t t = 0; t < order.size(); t++) {
      const Node& nd = nodes[order[t]];
      auto operand = [&](int id) -> uint32_t {
        const Node& o = nodes[id];
        if (o.op == 0) return pk::X_CONST | (uint32_t)o.cidx;
        if (o.op == 1) return pk::X_COL | ((uint32_t)o.col << 8) | (uint32_t)(o.rot + 128);
        if (at[id] + 1 == (int)t) return pk::X_PREV;
        return pk::X_SLOT | (uint32_t)slot_of[id];
      };
      const uint32_t a = operand(nd.a), b = operand(nd.b);
      // operands dying here free their slots before the destination is chosen (the kernel reads both first)
      for (int src : {nd.a, nd.b})
        if (nodes[src].op >= 2 && last_use[src] == (int)t && slot_of[src] >= 0) {
          free_slots.push_back((uint32_t)slot_of[src]);
          slot_of[src] = -2;
        }
      uint32_t dst = pk::X_NO_STORE;
      if (wants_slot[order[t]]) {
        if (!free_slots.empty()) {
          dst = free_slots.back();
          free_slots.pop_back();
        } else {
          dst = nslots++;
        }
        slot_of[order[t]] = (int)dst;
      }
      double bd = nd.op == 4 ? bound[nd.a] * bound[nd.b] / 128.0 + 1.0 : bound[nd.a] + bound[nd.b];
      if (nd.op != 4 && bd > pk::EXPR_VALUE_BOUND) {
        code.push_back({((uint32_t)(nd.op - 2) << 24) | pk::X_NO_STORE, a, b});
        code.push_back({(2u << 24) | dst, pk::X_PREV, one_operand});
        bd = bd / 128.0 + 1.0;
        nreduce++;
      } else {
        code.push_back({((uint32_t)(nd.op - 2) << 24) | dst, a, b});
      }
      bound[order[t]] = bd;
    }
    if (nslots == 0) nslots = 1;
  }
  // six u32 -- instructions, products, column reads, live-value slots, constants, inserted reductions -- then the code
  // (12 bytes per instruction): what the test hooks report
  std::vector<uint8_t> report() const {
    uint32_t st[6] = {(uint32_t)code.size(), 0, 0, nslots, (uint32_t)consts.size(), nreduce};
    for (auto& ins : code) {
      if ((ins.op_dst >> 24) == 2) st[1]++;
      if ((ins.a & (3u << 30)) == pk::X_COL) st[2]++;
      if ((ins.b & (3u << 30)) == pk::X_COL) st[2]++;
    }
    std::vector<uint8_t> r(24 + code.size() * sizeof(pk::XInstr));
    memcpy(r.data(), st, 24);
    memcpy(r.data() + 24, code.data(), code.size() * sizeof(pk::XInstr));
    return r;
  }
};

// expr_kernel over en rows of `count` proofs (grid.y = proof): one program and one set of row masks; proof p's column
// pointers at ptrs[p masks.size() ...], its constants (c, patched for the proof) at consts[p nconsts ...], uploaded in the
// kernel's working form c 2^261, its result at out + p en; the LDS of the slots beyond the registers is checked against
// what one workgroup may hold before anything is uploaded or launched.  create_proofs and the test hook
// h2_selftest_expr_run (count = 1) both launch the quotient program through here.
inline size_t expr_lds_bytes(const ExprProgram& X) {
  const size_t lds_slots = X.nslots > (uint32_t)pk::EXPR_REG_SLOTS ? X.nslots - pk::EXPR_REG_SLOTS : 1;
  const size_t lds = lds_slots * 9 * pk::EXPR_BLOCK * 4;
  if (lds > pk::EXPR_LDS_MAX) fail(H2_EINVAL, "quotient program needs too many live values");
  return lds;
}
inline void expr_launch(Dev& d, const ExprProgram& X, const pk::XInstr* d_code, const std::vector<const U128*>& ptrs,
                        const std::vector<uint32_t>& masks, std::vector<Fr> consts, size_t nconsts, Col out, uint32_t step,
                        uint32_t en, size_t count) {
  const size_t lds = expr_lds_bytes(X);
  if (ptrs.size() != count * masks.size() || consts.size() != count * nconsts) fail(H2_EINVAL, "expr_launch: table sizes");
  const U128* const* d_ptrs = (const U128* const*)d.upload(ptrs.data(), ptrs.size() * sizeof(void*));
  const uint32_t* d_masks = (const uint32_t*)d.upload(masks.data(), masks.size() * 4);
  for (auto& c : consts)
    for (int t = 0; t < 5; t++) c = c + c;            // c 2^256 -> c 2^261: the kernel's working form (R' = 2^261)
  Col d_consts = d.upload_frs(consts);
  if (lds > 64 * 1024)                                // past 64 KiB: raised, as the MSM and NTT kernels raise theirs
    hip_ok(hipFuncSetAttribute((const void*)pk::expr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
           "hipFuncSetAttribute(expr_kernel)");
  hipLaunchKernelGGL(pk::expr_kernel, dim3((en + pk::EXPR_BLOCK - 1) / pk::EXPR_BLOCK, (unsigned)count), dim3(pk::EXPR_BLOCK), lds,
                     d.s, d_code, (uint32_t)X.code.size(), d_ptrs, (uint32_t)masks.size(), d_masks, d_consts, (uint32_t)nconsts, out,
                     step, en);
  hip_ok(hipGetLastError(), "expr_kernel");
}

// a caller's expression DAG (the test hooks h2_selftest_host what = 7 and h2_selftest_expr_run): u32 node count, u32
// constant count, then per node four i32 {op, a, b, x} -- op 0: constant x; 1: column a at rotation x; 2 / 3 / 4: add /
// sub / mul of the earlier nodes a and b -- then the constants, 32 canonical little-endian bytes each.  The last node
// is the root.  Built through ExprProgram's own methods and compiled as the prover compiles its quotient.
inline void program_from_dag(const uint8_t* in, size_t in_len, ExprProgram& X) {
  if (!in || in_len < 8) fail(H2_EINVAL, "dag: truncated");
  uint32_t nn, nc;
  memcpy(&nn, in, 4);
  memcpy(&nc, in + 4, 4);
  if (nn == 0 || nn > (1u << 20) || nc > (1u << 20) || in_len != 8 + 16 * (size_t)nn + 32 * (size_t)nc)
    fail(H2_EINVAL, "dag: wrong length");
  std::vector<Fr> cs(nc);
  for (uint32_t j = 0; j < nc; j++)
    if (!Fr::from_le_bytes_canonical(in + 8 + 16 * (size_t)nn + 32 * (size_t)j, &cs[j])) fail(H2_EINVAL, "dag: constant not canonical");
  std::vector<int> id(nn);
  for (uint32_t i = 0; i < nn; i++) {
    int32_t f[4];
    memcpy(f, in + 8 + 16 * (size_t)i, 16);
    const int op = f[0], a = f[1], b = f[2], x = f[3];
    if (op == 0) {
      if (x < 0 || (uint32_t)x >= nc) fail(H2_EINVAL, "dag: no such constant");
      id[i] = X.constant(cs[x]);
    } else if (op == 1) {
      id[i] = X.column(a, x);                        // compile checks the column index and the rotation
    } else if (op >= 2 && op <= 4) {
      if (a < 0 || b < 0 || (uint32_t)a >= i || (uint32_t)b >= i) fail(H2_EINVAL, "dag: operand is not an earlier node");
      id[i] = op == 2 ? X.add(id[a], id[b]) : op == 3 ? X.sub(id[a], id[b]) : X.mul(id[a], id[b]);
    } else {
      fail(H2_EINVAL, "dag: unknown op");
    }
  }
  X.compile(id[nn - 1]);
}

}  // namespace product
}  // namespace h2
