// rowprog_compile.h -- what the run-time side (rowprog.hip) uses of the host-only row-program compiler (rowprog_compile.hip).
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "jit.h"
#include "rowprog_dev.cuh"

namespace srs {
namespace rowprog {

struct FieldOps {   // runtime-dispatched host field arithmetic
    int field;
    fe_t zero() const { return Fr::zero(); }
    fe_t one() const { return field == 0 ? Fr::one() : Fq::one(); }
    fe_t add(const fe_t &a, const fe_t &b) const { return field == 0 ? Fr::add(a, b) : Fq::add(a, b); }
    fe_t sub(const fe_t &a, const fe_t &b) const { return field == 0 ? Fr::sub(a, b) : Fq::sub(a, b); }
    fe_t mul(const fe_t &a, const fe_t &b) const { return field == 0 ? Fr::mul(a, b) : Fq::mul(a, b); }
    fe_t neg(const fe_t &a) const { return field == 0 ? Fr::neg(a) : Fq::neg(a); }
    fe_t halve(const fe_t &a) const { return field == 0 ? Fr::halve(a) : Fq::halve(a); }
    fe_t inv(const fe_t &a) const { return field == 0 ? Fr::inv(a) : Fq::inv(a); }
    fe_t from_u64(uint64_t v) const { return field == 0 ? Fr::from_u64(v) : Fq::from_u64(v); }
    bool is_zero(const fe_t &a) const { return Fr::is_zero(a); }
    bool eq(const fe_t &a, const fe_t &b) const { return Fr::eq(a, b); }
};

struct UOp {      // uniform program: u[dst] = op(u[a], u[b]);  leaves: constant / challenge
    int op;       // 0 const, 1 challenge(index), 2 add, 3 sub, 4 mul, 5 neg, 6 scaled copy: u[a] * 2^(5 b), b signed (sweep form)
    int a, b;
    fe_t c;
    int64_t chal;
};
struct VInsn {
    uint32_t op;
    int dst;      // virtual register
    int a, b;     // operands: >= 0 virtual reg; < 0: uniform index = -(x)-1 ; loads: a = column, b = rotation
};

struct Program {
    std::vector<UOp> uops;
    std::vector<Insn> insns;
    uint32_t result = 0, nslots = 1;
    Insn *d_insns = nullptr;        // device copy: filled by rowprog.hip (create)
    std::vector<VInsn> vins;        // SSA form (virtual registers), kept for emit_spec_source
    int result_vreg = -1;
    // "sweep" form (plan_sweep): the expression as a sum of terms coef * body, evaluated for ALL points per column load
    struct SweepTerm { int node; int coef; int sign; int level; };   // node: vreg, or -(u)-1 for a row-independent term; coef: uniform index (pre-scaled)
    struct SweepCluster { std::vector<int> terms, body, loads; bool linear = false; };     // body / loads: vregs in SSA order; linear: see plan_sweep
    std::vector<SweepTerm> sw_terms;
    std::vector<SweepCluster> sw_clusters;
    std::vector<int> sw_level;      // per vreg: power of 2^-5 its 9 x 29-bit value carries (field29.cuh: R' = 2^261 vs the ABI's 2^256)
    std::vector<int> sw_raise;      // [delta] -> uniform index of the raw constant 2^(261 - 5 delta): product with it adds delta levels
    int sw_one = -1;                // uniform index of 2^261 mod p (the radix' one): product with it folds a lazy value below 2p
    std::vector<int> sw_coef;       // the uniform entries that are term coefficients (dedicated entries: ProtoGalaxy scales them by the leaf weight)
    std::map<std::pair<int, int>, int> sw_uat;   // (uniform index, level) -> index of the copy scaled by 2^(-5 level) (operand of a body addition)
    bool sweep_ok = false;
    uint64_t fingerprint = 0;       // FNV-1a of the SSA program
    int spec_id = -1;               // index into the ahead-of-time specialised kernels, or -1: filled by rowprog.hip (kSpecs)
    jit::Kernel jit;                // straight-line kernel compiled at structure creation (jit.hip), or empty: filled by rowprog.hip
};

// straight-line C++ for the SSA program (one function template over the field) and for its sweep form (empty without one)
std::string emit_spec_source(const Program &p, const std::string &name, bool shared_mul);
std::string emit_sweep_source(const Program &p, const std::string &name, bool shared_mul);

// evaluate the uniform program for one point: challenge i -> ch[i] + pt * ch[i + fold_offset]
bool eval_uniform(const Program &p, const FieldOps &f, const fe_t *ch, size_t n_ch, size_t fold_offset, bool fold,
                  uint32_t pt, fe_t *out, std::string &err);

// inverse Vandermonde for the nodes first .. first + d, all rows: out[k * (d + 1) + j] = coefficient of X^k in L_j(X), k = 0..d
std::vector<fe_t> inverse_vandermonde_at(const FieldOps &f, size_t d, uint64_t first);
// rows 1..d of the matrix of the nodes 0..d: vinv[(k-1)*(d+1) + j] = coefficient of X^k in L_j(X)
inline std::vector<fe_t> inverse_vandermonde_rows(const FieldOps &f, size_t d) {
    std::vector<fe_t> m = inverse_vandermonde_at(f, d, 0);
    m.erase(m.begin(), m.begin() + (d + 1));
    return m;
}

// everything create() derives from the gate and lookup expressions alone (no device involved)
struct Compiled {
    size_t s_num_challenges = 0;   // PlonkStructure::num_challenges (compressed().num_challenges())
    size_t h_num_challenges = 0;   // homogeneous().num_challenges()  (challenge i folds with i + this)
    size_t degree = 0;             // homogeneous degree = number of cross terms
    Program cross;                 // homogeneous expression, fold mode
    Program plain_compressed;      // compressed expression, single witness (decider, plonk/mod.rs:328)
    Program plain_homogeneous;     // homogeneous expression, single witness (decider, sangria/mod.rs:351)
    std::vector<Program> lookup_progs;   // lookup_polys L_i then table_polys T_i (LookupEvalDomain: advice columns, challenges = [r])
    std::vector<Program> gate_progs;   // S.gates one by one (ProtoGalaxy leaves, plonk/mod.rs:697-701)
    size_t max_gate_degree = 0;    // max_i gates[i].degree()  (get_points_count, poly/mod.rs:535-545)
    std::vector<fe_t> vinv_g, vinv_g1;   // compute_G at integer points: inverse Vandermonde of the nodes 0..d_G (rows 1..d_G) / 1..d_G+1 (all rows)
    std::vector<fe_t> vinv;        // [degree][degree+1]
    int32_t min_rot = 0, max_rot = 0;           // range of the rotations of every column query in the gates / lookup expressions
};
// parse, compress, homogenise and compile; rc: 4 parse and argument errors, 7 index out of range (with false)
bool compile_structure(int field, size_t num_selectors, size_t num_fixed, size_t num_advice,
                       const uint64_t *gates, size_t gates_words, size_t num_gates, size_t num_lookups, bool has_vector_lookup,
                       const uint64_t *lookup_exprs, size_t lookup_words, Compiled &out, int &rc, std::string &err);

}  // namespace rowprog
}  // namespace srs
