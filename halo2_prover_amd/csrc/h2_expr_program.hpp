// h2_expr_program.hpp -- an expression DAG as a straight-line program: the compiler (host only, generic over the scalar
// field) of the kernel that interprets it (h2_expr_kernel.hpp, expr_kernel).  create_proof compiles its quotient
// numerator with it (h2_keygen.hpp), h2_expr_compile a caller's DAG (h2_capi.hip).
#pragma once
#include <algorithm>
#include <array>
#include <functional>
#include <map>
#include <tuple>

#include "h2_expr_kernel.hpp"
#include "h2_product_base.hpp"

namespace h2 {
namespace product {

// ---- a DAG compiled to a straight-line program (h2_expr_kernel.hpp expr_kernel) -------------------------------------------
template <class FP>
struct ExprProgramT {
  using Elem = HF<FP>;
  // nodes (hash-consed): 0 const, 1 column, 2 add, 3 sub, 4 mul
  struct Node {
    int op, a, b, col, rot, cidx;
    bool operator<(const Node& o) const {
      return std::tie(op, a, b, col, rot, cidx) < std::tie(o.op, o.a, o.b, o.col, o.rot, o.cidx);
    }
  };
  std::vector<Node> nodes;
  std::map<Node, int> index;
  std::vector<Elem> consts;            // constant table (the variables' entries are patched per proof / instance)
  std::map<std::array<uint8_t, 32>, int> const_index;
  int intern(const Node& nd) {
    auto it = index.find(nd);
    if (it != index.end()) return it->second;
    nodes.push_back(nd);
    index[nd] = (int)nodes.size() - 1;
    return (int)nodes.size() - 1;
  }
  int constant(const Elem& v) {
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
    consts.push_back(Elem::zero());
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
  // how many blocks share a CU (h2_expr_kernel.hpp, expr_kernel).
  void compile(int root) {
    for (const Node& nd : nodes)                     // the operand word has 22 bits for a column and 8 for rot + 128
      if (nd.op == 1 && (nd.col < 0 || nd.col >= (1 << 22) || nd.rot < -128 || nd.rot > 127))
        fail(H2_EINVAL, "quotient program: column index or rotation does not fit its operand word");
    (void)constant(Elem::one());                     // the reducing product's operand: interned before the node tables are sized
    // No recursion anywhere: a y-fold over all constraints is a chain as deep as the DAG is long (2^20 nodes through
    // h2_expr_compile).  An operand is always an earlier node (intern appends), so one forward pass numbers them all
    std::vector<int> need(nodes.size(), 0);
    for (size_t id = 0; id < nodes.size(); id++)
      if (nodes[id].op >= 2) {
        const int na = need[nodes[id].a], nb = need[nodes[id].b];
        need[id] = std::max(1, na == nb ? na + 1 : std::max(na, nb));
      }
    // depth first from the root on an explicit stack: a node is emitted once both operands are
    std::vector<int> order;
    std::vector<char> seen(nodes.size(), 0);
    std::vector<std::pair<int, int>> stack;          // (node, operands entered so far)
    seen[root] = 1;
    if (nodes[root].op >= 2) stack.push_back({root, 0});
    while (!stack.empty()) {
      const int id = stack.back().first, stage = stack.back().second++;
      const Node& nd = nodes[id];
      if (stage == 2) {
        order.push_back(id);
        stack.pop_back();
        continue;
      }
      const bool b_first = need[nd.b] > need[nd.a];
      const int next = (stage == 0) == b_first ? nd.b : nd.a;
      if (!seen[next]) {
        seen[next] = 1;
        if (nodes[next].op >= 2) stack.push_back({next, 0});
      }
    }
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
    // magnitudes in units of p (expr_kernel's header, which carries the argument for every field): constants are
    // canonical, columns within EXPR_COLUMN_BOUND, a product of a and b below a b EXPR_PRODUCT_SCALE + 1 (p^2 / 2^261 is at
    // most that scale times p); a sum that would pass EXPR_VALUE_BOUND is multiplied by one straight away
    std::vector<double> bound(nodes.size(), 0.0);
    for (size_t id = 0; id < nodes.size(); id++)
      if (nodes[id].op == 0) bound[id] = 1.0;
      else if (nodes[id].op == 1) bound[id] = pk::EXPR_COLUMN_BOUND;
    const uint32_t one_operand = pk::X_CONST | (uint32_t)nodes[constant(Elem::one())].cidx;
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
      double bd = nd.op == 4 ? bound[nd.a] * bound[nd.b] * pk::EXPR_PRODUCT_SCALE + 1.0 : bound[nd.a] + bound[nd.b];
      if (nd.op != 4 && bd > pk::EXPR_VALUE_BOUND) {
        code.push_back({((uint32_t)(nd.op - 2) << 24) | pk::X_NO_STORE, a, b});
        code.push_back({(2u << 24) | dst, pk::X_PREV, one_operand});
        bd = bd * pk::EXPR_PRODUCT_SCALE + 1.0;
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
  // report(), then the constant table (32 canonical little-endian bytes each; the one compile adds included)
  std::vector<uint8_t> report_with_table() const {
    std::vector<uint8_t> r = report();
    for (auto& c : consts) {
      uint8_t b[32];
      c.to_le_bytes(b);
      r.insert(r.end(), b, b + 32);
    }
    return r;
  }
};
using ExprProgram = ExprProgramT<BN254_FR>;    // the prover's: bn256::Fr

// the LDS of the slots beyond the registers, checked against what one workgroup may hold
template <class FP>
inline size_t expr_lds_bytes(const ExprProgramT<FP>& X) {
  const size_t lds = pk::expr_lds_for_slots(X.nslots);
  if (lds > pk::EXPR_LDS_MAX) fail(H2_EINVAL, "quotient program needs too many live values");
  return lds;
}

// A caller's expression DAG built through ExprProgramT's own methods and compiled as the prover compiles its quotient:
// nn nodes of four i32 {op, a, b, x} -- op 0: constant x of `cs`; 1: column a at rotation x; 2 / 3 / 4: add / sub / mul
// of the earlier nodes a and b; 5: variable x < n_vars -- the last node the root.  Every variable gets its own entry of
// the constant table, ahead of the constants (var_slot, if given, receives their indices).  A column index must be below
// n_cols.  public_rules: a root that is a leaf is multiplied by one (the test hooks refuse it, as they refuse op 5).
template <class FP>
inline void program_from_nodes(ExprProgramT<FP>& X, const int32_t* nd, size_t nn, const std::vector<HF<FP>>& cs, uint32_t n_cols,
                               uint32_t n_vars, bool public_rules, std::vector<uint32_t>* var_slot) {
  std::vector<int> var_node(n_vars);
  for (uint32_t v = 0; v < n_vars; v++) {
    int slot;
    var_node[v] = X.variable(&slot);
    if (var_slot) var_slot->push_back((uint32_t)slot);
  }
  std::vector<int> id(nn);
  for (size_t i = 0; i < nn; i++) {
    const int op = nd[4 * i], a = nd[4 * i + 1], b = nd[4 * i + 2], x = nd[4 * i + 3];
    if (op == 0) {
      if (x < 0 || (size_t)x >= cs.size()) fail(H2_EINVAL, "dag: no such constant");
      id[i] = X.constant(cs[x]);
    } else if (op == 1) {
      if (a >= 0 && (uint32_t)a >= n_cols) fail(H2_EINVAL, "dag: no such column");
      id[i] = X.column(a, x);                        // compile checks the operand word's column range and the rotation
    } else if (op >= 2 && op <= 4) {
      if (a < 0 || b < 0 || (size_t)a >= i || (size_t)b >= i) fail(H2_EINVAL, "dag: operand is not an earlier node");
      id[i] = op == 2 ? X.add(id[a], id[b]) : op == 3 ? X.sub(id[a], id[b]) : X.mul(id[a], id[b]);
    } else if (op == 5 && public_rules) {
      if (x < 0 || (uint32_t)x >= n_vars) fail(H2_EINVAL, "dag: no such variable");
      id[i] = var_node[x];
    } else {
      fail(H2_EINVAL, "dag: unknown op");
    }
  }
  int root = id[nn - 1];
  if (public_rules && X.nodes[root].op < 2) root = X.mul(root, X.constant(HF<FP>::one()));
  X.compile(root);
}

// the test hooks' DAG blob (h2_selftest_host what = 7 and h2_selftest_expr_run): u32 node count, u32 constant count,
// the nodes, then the constants, 32 canonical little-endian bytes each
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
  std::vector<int32_t> nd(4 * (size_t)nn);
  memcpy(nd.data(), in + 8, 16 * (size_t)nn);
  program_from_nodes<BN254_FR>(X, nd.data(), nn, cs, 1u << 22, 0, false, nullptr);
}

}  // namespace product
}  // namespace h2
