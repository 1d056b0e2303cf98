// rowprog_compile.hip -- the host-only compiler of the row programs rowprog.hip runs (no kernel, no HIP runtime call):
//   gate stream (include/sirius_amd.h, SRS_EX_*) -> Expression AST -> compressed + homogenised gate polynomial P
//   (src/plonk/util.rs:34-56, src/polynomial/expression.rs:356-429, src/plonk/mod.rs:68-121) -> SSA register program with CSE.
// P stays the small homogeneous expression (no symbolic blow-up: the cross terms are recovered numerically from its values
// at the points X = 0..d, see rowprog.hip).  Sub-expressions that do not depend on the row (constants, challenges, powers
// of u) become the uniform program, evaluated once per point on the host ("uniform table", eval_uniform); the row part is
// allocated to LDS slots for the interpreter, emitted as straight-line C++ (emit_spec_source) and planned and emitted in
// sweep form (plan_sweep, emit_sweep_source) for the ahead-of-time (tools/gen_rowprog_spec.py) and run-time compiled kernels.
// Everything here is deterministic text and vectors: compile_structure is the one entry point create() calls.
#include "rowprog_compile.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <tuple>

namespace srs {
namespace rowprog {

namespace {

// ---------------------------------------------------------------------------------------------
// host: Expression AST (reference src/polynomial/expression.rs:112-120)
// ---------------------------------------------------------------------------------------------
enum NodeKind { N_CONST, N_POLY, N_CHAL, N_NEG, N_SUM, N_PROD, N_SCALED };
struct Node {
    int kind;
    fe_t c;           // N_CONST / N_SCALED
    int64_t index;    // N_POLY / N_CHAL
    int32_t rot;      // N_POLY
    int a, b;
};
struct Ast {
    std::vector<Node> n;
    int add(int kind, int a = -1, int b = -1, int64_t index = 0, int32_t rot = 0, const fe_t *c = nullptr) {
        Node x;
        x.kind = kind;
        x.a = a;
        x.b = b;
        x.index = index;
        x.rot = rot;
        std::memset(&x.c, 0, sizeof(x.c));
        if (c) x.c = *c;
        n.push_back(x);
        return (int)n.size() - 1;
    }
};

// gate stream: postfix words, see include/sirius_amd.h (SRS_EX_*)
static bool parse_gates(const uint64_t *w, size_t nw, size_t num_gates, Ast &ast, std::vector<int> &roots, std::string &err) {
    std::vector<int> st;
    size_t i = 0;
    while (i < nw) {
        uint64_t op = w[i++];
        switch (op) {
        case 0: {   // CONST c[4]
            if (i + 4 > nw) { err = "truncated constant"; return false; }
            fe_t c;
            std::memcpy(&c, &w[i], 32);
            i += 4;
            st.push_back(ast.add(N_CONST, -1, -1, 0, 0, &c));
            break;
        }
        case 1: {   // POLY index rot
            if (i + 2 > nw) { err = "truncated query"; return false; }
            st.push_back(ast.add(N_POLY, -1, -1, (int64_t)w[i], (int32_t)(int64_t)w[i + 1]));
            i += 2;
            break;
        }
        case 2:
            if (i + 1 > nw) { err = "truncated challenge"; return false; }
            st.push_back(ast.add(N_CHAL, -1, -1, (int64_t)w[i]));
            i += 1;
            break;
        case 3:
            if (st.empty()) { err = "stack underflow"; return false; }
            st.back() = ast.add(N_NEG, st.back());
            break;
        case 4:
        case 5: {
            if (st.size() < 2) { err = "stack underflow"; return false; }
            int b = st.back();
            st.pop_back();
            int a = st.back();
            st.back() = ast.add(op == 4 ? N_SUM : N_PROD, a, b);
            break;
        }
        case 6: {
            if (st.empty() || i + 4 > nw) { err = "bad scaled"; return false; }
            fe_t c;
            std::memcpy(&c, &w[i], 32);
            i += 4;
            st.back() = ast.add(N_SCALED, st.back(), -1, 0, 0, &c);
            break;
        }
        case 7:
            if (st.size() != 1) { err = "gate expression does not reduce to one value"; return false; }
            roots.push_back(st.back());
            st.clear();
            break;
        default:
            err = "unknown expression opcode";
            return false;
        }
    }
    if (!st.empty() || roots.size() != num_gates) { err = "gate count mismatch"; return false; }
    return true;
}

static void collect_challenges(const Ast &ast, int r, std::vector<int64_t> &set) {
    const Node &x = ast.n[r];
    if (x.kind == N_CHAL) {
        if (std::find(set.begin(), set.end(), x.index) == set.end()) set.push_back(x.index);
    }
    if (x.a >= 0) collect_challenges(ast, x.a, set);
    if (x.b >= 0) collect_challenges(ast, x.b, set);
}
static size_t num_challenges(const Ast &ast, int r) {   // Expression::num_challenges, expression.rs:163-167
    std::vector<int64_t> set;
    collect_challenges(ast, r, set);
    return set.size();
}

// compress_expression (src/plonk/util.rs:34-56)
static int compress(Ast &ast, const std::vector<int> &gates, size_t challenge_index, const FieldOps &f) {
    fe_t z = f.zero();
    if (gates.size() > 1) {
        int acc = ast.add(N_CONST, -1, -1, 0, 0, &z);
        for (int g : gates) {
            int y = ast.add(N_CHAL, -1, -1, (int64_t)challenge_index);
            acc = ast.add(N_SUM, g, ast.add(N_PROD, acc, y));
        }
        return acc;
    }
    if (gates.size() == 1) return gates[0];
    return ast.add(N_CONST, -1, -1, 0, 0, &z);
}

static int challenge_in_degree(Ast &ast, size_t idx, size_t degree) {   // expression.rs:501-513
    int r = ast.add(N_CHAL, -1, -1, (int64_t)idx);
    for (size_t i = 2; i <= degree; ++i) r = ast.add(N_PROD, r, ast.add(N_CHAL, -1, -1, (int64_t)idx));
    return r;
}

// Expression::homogeneous (src/polynomial/expression.rs:356-429)
struct Ctx {
    size_t num_selectors, num_fixed, num_advice, num_challenges;
    size_t num_lookups = 0;     // each adds the 5 fold variables (l, t, m, h, g) after the advice columns
    size_t num_fold_vars() const { return num_advice + 5 * num_lookups; }   // expression.rs:61-63
    // Column of fold variable j inside the CONCATENATED witness W[0] || W[1] (|| W[2]).  This is index_map of
    // PlonkEvalDomain::eval_advice_var (src/plonk/eval.rs:169-201) composed with the round sizes of
    // ConstraintSystemMetainfo::build (constraint_system_metainfo.rs:58-79): in both the 2-round and the
    // 3-round layout (l,t,m) of lookup li sits at columns num_advice + 3 li + {0,1,2} and (h,g) at
    // num_advice + 3 L + 2 li + {0,1}.
    size_t witness_col(size_t j) const {
        if (j < num_advice) return j;
        size_t li = (j - num_advice) / 5, sub = (j - num_advice) % 5;
        return sub < 3 ? num_advice + li * 3 + sub : num_advice + 3 * num_lookups + li * 2 + (sub - 3);
    }
};
static bool homogeneous(Ast &ast, int r, const Ctx &ctx, int &out, size_t &degree, std::string &err) {
    const Node x = ast.n[r];
    switch (x.kind) {
    case N_CONST: out = r; degree = 0; return true;
    case N_POLY: {
        size_t i = (size_t)x.index;
        if (i < ctx.num_selectors + ctx.num_fixed) degree = 0;
        else if (i < ctx.num_selectors + ctx.num_fixed + ctx.num_fold_vars()) degree = 1;   // Advice | Lookup
        else { err = "unknown query index " + std::to_string(i); return false; }
        out = r;
        return true;
    }
    case N_CHAL: out = r; degree = 1; return true;
    case N_NEG: {
        int a; if (!homogeneous(ast, x.a, ctx, a, degree, err)) return false;
        out = ast.add(N_NEG, a);
        return true;
    }
    case N_SCALED: {
        int a; if (!homogeneous(ast, x.a, ctx, a, degree, err)) return false;
        out = ast.add(N_SCALED, a, -1, 0, 0, &x.c);
        return true;
    }
    case N_PROD: {
        int a, b; size_t da, db;
        if (!homogeneous(ast, x.a, ctx, a, da, err) || !homogeneous(ast, x.b, ctx, b, db, err)) return false;
        out = ast.add(N_PROD, a, b);
        degree = da + db;
        return true;
    }
    default: {   // N_SUM
        int a, b; size_t da, db;
        if (!homogeneous(ast, x.a, ctx, a, da, err) || !homogeneous(ast, x.b, ctx, b, db, err)) return false;
        if (da > db) {
            out = ast.add(N_SUM, a, ast.add(N_PROD, b, challenge_in_degree(ast, ctx.num_challenges, da - db)));
            degree = da;
        } else if (da < db) {
            out = ast.add(N_SUM, ast.add(N_PROD, a, challenge_in_degree(ast, ctx.num_challenges, db - da)), b);
            degree = db;
        } else {
            out = ast.add(N_SUM, a, b);
            degree = da;
        }
        return true;
    }
    }
}

// Expression::degree (src/polynomial/expression.rs:431-447)
static size_t expr_degree(const Ast &ast, int r, const Ctx &ctx) {
    const Node &x = ast.n[r];
    switch (x.kind) {
    case N_CONST: return 0;
    case N_POLY: {
        size_t i = (size_t)x.index;
        return (i >= ctx.num_selectors + ctx.num_fixed) ? 1 : 0;
    }
    case N_CHAL: return 1;
    case N_NEG:
    case N_SCALED: return expr_degree(ast, x.a, ctx);
    case N_SUM: return std::max(expr_degree(ast, x.a, ctx), expr_degree(ast, x.b, ctx));
    default: return expr_degree(ast, x.a, ctx) + expr_degree(ast, x.b, ctx);
    }
}

// ---------------------------------------------------------------------------------------------
// host: compile an expression into (uniform program, row program)
// ---------------------------------------------------------------------------------------------
// A value is either
//   KNOWN   : compile-time constant (folded)                 -> becomes a uniform-table entry
//   UNIFORM : depends on challenges only (evaluated per call, per point on the host)
//   ROW     : depends on the row (virtual register)
struct Val {
    int cls;      // 0 known, 1 uniform, 2 row
    int id;       // uniform index / virtual register
    fe_t k;       // known value
};

struct Compiler {
    const Ast &ast;
    FieldOps f;
    Ctx ctx;
    bool fold_mode;                 // true: advice/challenges are W1 + X*W2 (cross terms); false: plain
    std::vector<UOp> uops;
    std::vector<VInsn> vins;
    int nvreg = 0;
    std::map<int, Val> memo;                                     // AST node -> value
    std::map<std::tuple<int, int, int>, int> u_cse;              // (op, a, b) -> uniform index
    std::map<std::tuple<uint32_t, int, int>, int> r_cse;         // (op, a, b) -> vreg
    std::map<std::tuple<int64_t, int>, int> chal_cse;
    std::string err;

    Compiler(const Ast &a, FieldOps fo, Ctx c, bool fm) : ast(a), f(fo), ctx(c), fold_mode(fm) {}

    int u_const(const fe_t &c) {
        for (size_t i = 0; i < uops.size(); ++i)
            if (uops[i].op == 0 && f.eq(uops[i].c, c)) return (int)i;
        UOp u{};
        u.op = 0;
        u.c = c;
        uops.push_back(u);
        return (int)uops.size() - 1;
    }
    int u_chal(int64_t idx) {
        auto key = std::make_tuple(idx, 0);
        auto it = chal_cse.find(key);
        if (it != chal_cse.end()) return it->second;
        UOp u{};
        u.op = 1;
        u.chal = idx;
        uops.push_back(u);
        return chal_cse[key] = (int)uops.size() - 1;
    }
    int u_op(int op, int a, int b) {
        if ((op == 2 || op == 4) && a > b) std::swap(a, b);
        auto key = std::make_tuple(op, a, b);
        auto it = u_cse.find(key);
        if (it != u_cse.end()) return it->second;
        UOp u{};
        u.op = op;
        u.a = a;
        u.b = b;
        uops.push_back(u);
        return u_cse[key] = (int)uops.size() - 1;
    }
    Val known(const fe_t &k) { Val v; v.cls = 0; v.id = -1; v.k = k; return v; }
    Val uniform(int id) { Val v{}; v.cls = 1; v.id = id; return v; }
    Val rowv(int id) { Val v{}; v.cls = 2; v.id = id; return v; }
    int as_uniform(const Val &v) { return v.cls == 0 ? u_const(v.k) : v.id; }
    int operand(const Val &v) { return v.cls == 2 ? v.id : -(as_uniform(v)) - 1; }
    Val r_op(uint32_t op, int a, int b) {
        if ((op == I_ADD || op == I_MUL) && a > b) std::swap(a, b);
        auto key = std::make_tuple(op, a, b);
        auto it = r_cse.find(key);
        if (it != r_cse.end()) return rowv(it->second);
        VInsn in{op, nvreg++, a, b};
        vins.push_back(in);
        r_cse[key] = in.dst;
        return rowv(in.dst);
    }

    Val v_add(const Val &a, const Val &b) {
        if (a.cls == 0 && b.cls == 0) return known(f.add(a.k, b.k));
        if (a.cls == 0 && f.is_zero(a.k)) return b;
        if (b.cls == 0 && f.is_zero(b.k)) return a;
        if (a.cls < 2 && b.cls < 2) return uniform(u_op(2, as_uniform(a), as_uniform(b)));
        return r_op(I_ADD, operand(a), operand(b));
    }
    Val v_neg(const Val &a) {
        if (a.cls == 0) return known(f.neg(a.k));
        if (a.cls == 1) return uniform(u_op(5, a.id, -1));
        return r_op(I_NEG, a.id, 0);
    }
    Val v_mul(const Val &a, const Val &b) {
        if (a.cls == 0 && b.cls == 0) return known(f.mul(a.k, b.k));
        if ((a.cls == 0 && f.is_zero(a.k)) || (b.cls == 0 && f.is_zero(b.k))) return known(f.zero());
        if (a.cls == 0 && f.eq(a.k, f.one())) return b;
        if (b.cls == 0 && f.eq(b.k, f.one())) return a;
        if (a.cls < 2 && b.cls < 2) return uniform(u_op(4, as_uniform(a), as_uniform(b)));
        if (a.cls == 2 && b.cls == 2 && a.id == b.id) return r_op(I_SQR, a.id, 0);
        return r_op(I_MUL, operand(a), operand(b));
    }

    Val walk(int r) {
        auto it = memo.find(r);
        if (it != memo.end()) return it->second;
        const Node &x = ast.n[r];
        Val v;
        switch (x.kind) {
        case N_CONST: v = known(x.c); break;
        case N_CHAL: v = uniform(u_chal(x.index)); break;
        case N_POLY: {
            size_t i = (size_t)x.index;
            uint32_t op;
            int col;
            if (i < ctx.num_selectors) { op = I_LD_SEL; col = (int)i; }
            else if (i < ctx.num_selectors + ctx.num_fixed) { op = I_LD_FIX; col = (int)(i - ctx.num_selectors); }
            else if (i < ctx.num_selectors + ctx.num_fixed + ctx.num_fold_vars()) { op = I_LD_ADV; col = (int)ctx.witness_col(i - ctx.num_selectors - ctx.num_fixed); }
            else { err = "column index " + std::to_string(i) + " out of range"; v = known(f.zero()); break; }
            auto key = std::make_tuple(op, col, (int)x.rot);
            auto c = r_cse.find(key);
            if (c != r_cse.end()) { v = rowv(c->second); break; }
            VInsn in{op, nvreg++, col, (int)x.rot};
            vins.push_back(in);
            r_cse[key] = in.dst;
            v = rowv(in.dst);
            break;
        }
        case N_NEG: v = v_neg(walk(x.a)); break;
        case N_SUM: { Val a = walk(x.a); Val b = walk(x.b); v = v_add(a, b); break; }
        case N_PROD: { Val a = walk(x.a); Val b = walk(x.b); v = v_mul(a, b); break; }
        default: { Val a = walk(x.a); v = v_mul(a, known(x.c)); break; }
        }
        memo[r] = v;
        return v;
    }
};

// linear-scan allocation of virtual registers to LDS slots
static bool allocate(const std::vector<VInsn> &vins, int nvreg, int result_vreg, std::vector<Insn> &out,
                     uint32_t &result_code, uint32_t &nslots) {
    std::vector<int> last(nvreg, -1);
    for (size_t i = 0; i < vins.size(); ++i) {
        const VInsn &in = vins[i];
        if (in.op > I_LD_ADV) {
            if (in.a >= 0) last[in.a] = (int)i;
            if (in.op <= I_MUL && in.b >= 0) last[in.b] = (int)i;
        }
    }
    if (result_vreg >= 0) last[result_vreg] = (int)vins.size();
    std::vector<int> slot(nvreg, -1);
    std::vector<int> free_list;
    uint32_t n = 0;
    auto enc = [&](int x) -> uint32_t { return x >= 0 ? (uint32_t)slot[x] : (UNIFORM_BIT | (uint32_t)(-x - 1)); };
    for (size_t i = 0; i < vins.size(); ++i) {
        const VInsn &in = vins[i];
        Insn o;
        o.op = in.op;
        if (in.op <= I_LD_ADV) {
            o.a = (uint32_t)in.a;
            o.b = (uint32_t)in.b;
        } else {
            o.a = enc(in.a);
            o.b = in.op <= I_MUL ? enc(in.b) : 0;
            // operands dying here free their slots before the destination is chosen
            if (in.a >= 0 && last[in.a] == (int)i) free_list.push_back(slot[in.a]);
            if (in.op <= I_MUL && in.b >= 0 && in.b != in.a && last[in.b] == (int)i) free_list.push_back(slot[in.b]);
        }
        int s;
        if (!free_list.empty()) { s = free_list.back(); free_list.pop_back(); } else s = (int)n++;
        slot[in.dst] = s;
        o.dst = (uint32_t)s;
        out.push_back(o);
        if (last[in.dst] < 0) free_list.push_back(s);   // dead value (cannot happen after CSE, but stay safe)
    }
    nslots = n ? n : 1;
    result_code = result_vreg >= 0 ? (uint32_t)slot[result_vreg] : 0;
    return true;
}

static uint64_t fingerprint_of(const Program &p) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xff; h *= 1099511628211ull; } };
    for (auto &in : p.vins) { mix(in.op); mix((uint64_t)(int64_t)in.dst); mix((uint64_t)(int64_t)in.a); mix((uint64_t)(int64_t)in.b); }
    mix((uint64_t)(int64_t)p.result_vreg);
    mix(p.result);
    mix(p.uops.size());
    return h;
}

}  // namespace

// straight-line C++ for the SSA program (one function template over the field)
std::string emit_spec_source(const Program &p, const std::string &name, bool shared_mul) {
    std::string o;
    auto opnd = [](int x) { return x >= 0 ? "v" + std::to_string(x) : "U[" + std::to_string(-x - 1) + "]"; };
    // shared_mul: the multiplications call ONE shared body (mul_ni / sqr_ni, rowprog_dev.cuh) instead of inlining 2 KB of
    // code each, so a program is tens of KB, not hundreds.  Run-time compiled kernels need that: with every multiplier
    // inlined they ran 30 % slower than the same ISA linked into the library (profiles/r01_jit_vs_aot.txt), called they
    // match it.  The ahead-of-time kernels keep the inlined form (3 % faster there).
    const std::string MUL = shared_mul ? "mul_ni<F>(" : "F::mul(", SQR = shared_mul ? "sqr_ni<F>(" : "F::sqr(";
    o += "template <class F>\n__device__ __forceinline__ fe_t " + name +
         "(const RowCtx &C, uint32_t row, uint32_t pt, const fe_t *__restrict__ U) {\n";
    o += "    const uint32_t mask = C.rows - 1; (void)mask; (void)pt; (void)U;\n";
    for (auto &in : p.vins) {
        std::string d = "    const fe_t v" + std::to_string(in.dst) + " = ";
        std::string rr = "(row + " + std::to_string((uint32_t)in.b) + "u) & mask";
        switch (in.op) {
        case I_LD_SEL: o += d + "ld_sel<F>(C, " + std::to_string(in.a) + ", " + rr + ");\n"; break;
        case I_LD_FIX: o += d + "ld_fix<F>(C, " + std::to_string(in.a) + ", " + rr + ");\n"; break;
        case I_LD_ADV: o += d + "ld_adv<F>(C, " + std::to_string(in.a) + ", " + rr + ", pt);\n"; break;
        case I_ADD: o += d + "F::add(" + opnd(in.a) + ", " + opnd(in.b) + ");\n"; break;
        case I_SUB: o += d + "F::sub(" + opnd(in.a) + ", " + opnd(in.b) + ");\n"; break;
        case I_MUL: o += d + MUL + opnd(in.a) + ", " + opnd(in.b) + ");\n"; break;
        case I_SQR: o += d + SQR + opnd(in.a) + ");\n"; break;
        case I_DBL: o += d + "F::dbl(" + opnd(in.a) + ");\n"; break;
        default: o += d + "F::neg(" + opnd(in.a) + ");\n"; break;
        }
    }
    if (p.result_vreg >= 0) o += "    return v" + std::to_string(p.result_vreg) + ";\n";
    else o += "    return U[" + std::to_string(p.result & ~UNIFORM_BIT) + "];\n";
    o += "}\n";
    return o;
}

namespace {

// ---------------------------------------------------------------------------------------------
// Sweep form.  The straight-line program above evaluates ONE point per pass over the row's columns: d + 1 passes, each
// re-reading every column from L2 / HBM (profiles/r01_pmc_step_kernels.json: 6.3x the algorithmic bytes).  The sweep form
// turns the loops inside out: the expression is flattened into a sum of TERMS  coef(pt) * body(row, pt)  -- the linear
// skeleton (+, -, scaling by row-independent values) is distributed, the coefficients become new entries of the uniform
// table (host work per call) -- and terms sharing columns form CLUSTERS.  A cluster loads its columns once, then loops
// over the points: advice leaves are affine in the point (W1 + X W2, or the Lagrange fold (w0 + w1)/2 + X (w0 - w1)/2), so the
// next point costs one addition per leaf; the per-point accumulators live in LDS.  Bodies run on the 9 x 29-bit
// multiplier (field29.cuh), whose Montgomery radix 2^261 differs from the ABI's 2^256: a product of two ABI-form values
// comes out 2^-5 short ("level" + 1).  Levels are tracked statically; the term's final multiplication by its coefficient
// uses a coefficient pre-scaled by 2^(5 (level + 1)) on the host, which lands every term back in ABI form -- the sum is
// the same field element as the straight-line program's, canonical, bit for bit.
// ---------------------------------------------------------------------------------------------
struct SweepBuilder {
    Program &p;
    std::map<std::tuple<int, int, int>, int> cse;          // (op, a, b) -> uniform index, for the entries created here
    std::vector<int> def;                                  // vreg -> index into p.vins
    explicit SweepBuilder(Program &prog) : p(prog) {
        int nv = 0;
        for (auto &in : p.vins) nv = std::max(nv, in.dst + 1);
        def.assign(nv, -1);
        for (size_t i = 0; i < p.vins.size(); ++i) def[p.vins[i].dst] = (int)i;
    }
    int uop(int op, int a, int b, const fe_t *c = nullptr) {
        if (op == 4 && a > b) std::swap(a, b);
        auto key = std::make_tuple(op, a, b);
        if (!c) { auto it = cse.find(key); if (it != cse.end()) return it->second; }
        UOp u{};
        u.op = op;
        u.a = a;
        u.b = b;
        if (c) u.c = *c;
        p.uops.push_back(u);
        const int id = (int)p.uops.size() - 1;
        if (!c) cse[key] = id;
        return id;
    }
    int u_mul(int a, int b) { return a < 0 ? b : (b < 0 ? a : uop(4, a, b)); }      // -1 = coefficient one
    int u_scaled(int a, int e) { return e == 0 ? a : uop(6, a, e); }
    int one = -1;
    int u_one(const FieldOps &f) {
        if (one < 0) { fe_t o = f.one(); one = uop(0, 0, 0, &o); }
        return one;
    }
    int two = -1;
    int u_two(const FieldOps &f) {
        if (two < 0) { fe_t t = f.add(f.one(), f.one()); two = uop(0, 0, 0, &t); }
        return two;
    }
    bool is_linear_mul(const VInsn &in) const { return in.op == I_MUL && ((in.a < 0) != (in.b < 0)); }

    // distribute the linear skeleton below `x` (operand code) with coefficient `coef` (uniform index or -1) and sign
    void lin(int x, int coef, int sign, const FieldOps &f, int depth) {
        if (x < 0) {                                         // row-independent value
            p.sw_terms.push_back({x, coef, sign, 0});
            return;
        }
        const VInsn &in = p.vins[def[x]];
        if (depth < 64) {
            switch (in.op) {
            case I_ADD: lin(in.a, coef, sign, f, depth + 1); lin(in.b, coef, sign, f, depth + 1); return;
            case I_SUB: lin(in.a, coef, sign, f, depth + 1); lin(in.b, coef, -sign, f, depth + 1); return;
            case I_NEG: lin(in.a, coef, -sign, f, depth + 1); return;
            case I_DBL: lin(in.a, u_mul(coef, u_two(f)), sign, f, depth + 1); return;
            case I_MUL:
                if (is_linear_mul(in)) {
                    const int u = in.a < 0 ? -in.a - 1 : -in.b - 1, v = in.a < 0 ? in.b : in.a;
                    lin(v, u_mul(coef, u), sign, f, depth + 1);
                    return;
                }
                break;
            default: break;
            }
        }
        p.sw_terms.push_back({x, coef, sign, 0});
    }
    // level of a body value; uniform operands of body additions are re-scaled on the host, so they never raise a level
    int level_of(int v) {
        if (p.sw_level[v] >= 0) return p.sw_level[v];
        const VInsn &in = p.vins[def[v]];
        int l = 0;
        auto lv = [&](int x) { return x < 0 ? 0 : level_of(x); };
        switch (in.op) {
        case I_LD_SEL: case I_LD_FIX: case I_LD_ADV: l = 0; break;
        case I_MUL: l = lv(in.a) + lv(in.b) + 1; break;
        case I_SQR: l = 2 * lv(in.a) + 1; break;
        case I_ADD: case I_SUB: l = std::max(lv(in.a), lv(in.b)); break;
        default: l = lv(in.a); break;
        }
        return p.sw_level[v] = l;
    }
    void collect(int v, std::vector<char> &seen, std::vector<int> &body, std::vector<int> &loads) {
        if (v < 0 || seen[v]) return;
        seen[v] = 1;
        const VInsn &in = p.vins[def[v]];
        if (in.op <= I_LD_ADV) { loads.push_back(v); return; }
        collect(in.a, seen, body, loads);
        if (in.op <= I_MUL) collect(in.b, seen, body, loads);
        body.push_back(v);
    }
};

// registers a cluster may spend on hoisted column values: an advice leaf is (value, step) = 16 VGPRs, a fixed one 8
static constexpr int SWEEP_LOAD_BUDGET = 112;

static void plan_sweep(Program &p, const FieldOps &f) {
    p.sweep_ok = false;
    p.sw_terms.clear();
    p.sw_clusters.clear();
    if (p.result_vreg < 0 || p.vins.empty()) return;
    SweepBuilder B(p);
    B.lin(p.result_vreg, -1, +1, f, 0);
    if (p.sw_terms.empty() || p.sw_terms.size() > 4096) { p.sw_terms.clear(); return; }
    p.sw_level.assign(B.def.size(), -1);
    for (auto &t : p.sw_terms) {
        t.level = t.node < 0 ? 0 : B.level_of(t.node);
        if (t.level > 40) { p.sw_terms.clear(); return; }
        if (t.node < 0) {                                    // constant term: coefficient * value, a dedicated ABI-form entry
            t.coef = B.uop(6, B.u_mul(t.coef, -t.node - 1), 0);
        } else {                                             // coef * 2^(5 (level + 1)): the closing product returns to ABI form
            t.coef = B.u_scaled(t.coef < 0 ? B.u_one(f) : t.coef, t.level + 1);
        }
    }
    p.sw_coef.clear();
    for (auto &t : p.sw_terms) p.sw_coef.push_back(t.coef);
    std::sort(p.sw_coef.begin(), p.sw_coef.end());
    p.sw_coef.erase(std::unique(p.sw_coef.begin(), p.sw_coef.end()), p.sw_coef.end());
    // helper constants of the 2^261-radix bodies
    int max_level = 0;
    for (int l : p.sw_level) max_level = std::max(max_level, l);
    {                                                        // a constant of its own (never shared with a coefficient entry)
        fe_t c = f.one();
        for (int k = 0; k < 5; ++k) c = f.add(c, c);
        p.sw_one = B.uop(0, 0, 0, &c);
    }
    p.sw_raise.assign(max_level + 1, -1);
    for (int d = 1; d <= max_level; ++d) p.sw_raise[d] = B.u_scaled(B.u_one(f), 1 - d);
    p.sw_uat.clear();
    for (size_t i = 0; i < p.vins.size(); ++i) {            // uniform operands of body additions at level > 0
        const VInsn &in = p.vins[i];
        if ((in.op != I_ADD && in.op != I_SUB) || p.sw_level[in.dst] <= 0) continue;
        for (int x : {in.a, in.b})
            if (x < 0) p.sw_uat[{-x - 1, p.sw_level[in.dst]}] = B.u_scaled(-x - 1, -p.sw_level[in.dst]);
    }
    // Terms that are AFFINE in the evaluation point -- a product chain with at most one advice leaf and point-independent
    // coefficients (no challenge in the uniform program: the ProtoGalaxy gate polynomials) -- need no evaluation per point: their
    // clusters compute the value at the first point and the slope (the same chain with the leaf's step in place of its value)
    // once, and every further point is one lazy addition.  chain(v) = number of advice leaves of a pure product chain, -1 otherwise.
    bool const_u = true;
    for (const UOp &u : p.uops) const_u = const_u && u.op != 1;
    std::function<int(int)> chain = [&](int v) -> int {
        if (v < 0) return 0;
        const VInsn &in = p.vins[B.def[v]];
        if (in.op == I_LD_ADV) return 1;
        if (in.op == I_LD_SEL || in.op == I_LD_FIX) return 0;
        if (in.op != I_MUL) return -1;
        const int a = chain(in.a), b = chain(in.b);
        return (a < 0 || b < 0) ? -1 : a + b;
    };
    std::vector<char> term_linear(p.sw_terms.size(), 0);
    for (size_t ti = 0; ti < p.sw_terms.size(); ++ti) {
        if (!const_u) break;
        const auto &t = p.sw_terms[ti];
        const int c = t.node < 0 ? 0 : chain(t.node);
        term_linear[ti] = c == 0 || c == 1;
    }
    // clusters: terms in expression order; a term joins the open cluster while the hoisted columns fit the budget
    const size_t nv = B.def.size();
    std::vector<char> in_cluster(nv, 0);
    Program::SweepCluster cur;
    int cost = 0;
    auto load_cost = [&](int v) { return p.vins[B.def[v]].op == I_LD_ADV ? 16 : 8; };
    // a term q * (s * y) keeps the hoisted affine factor q s and its step in registers across the point loop (emit_sweep_source):
    // 18 VGPRs, while the fixed leaf q is only needed before the loop
    constexpr int hoist_regs = 10;
    auto hoist_cost = [&](int v) -> int {
        if (v < 0) return 0;
        const VInsn &in = p.vins[B.def[v]];
        if (in.op != I_MUL) return 0;
        for (int o1 = 0; o1 < 2; ++o1) {
            const int a = o1 ? in.b : in.a, u = o1 ? in.a : in.b;
            if (a < 0 || u < 0) continue;
            const int oa = p.vins[B.def[a]].op, ou = p.vins[B.def[u]].op;
            if ((oa != I_LD_FIX && oa != I_LD_SEL) || ou != I_MUL) continue;
            const VInsn &iu = p.vins[B.def[u]];
            for (int x : {iu.a, iu.b})
                if (x >= 0 && p.vins[B.def[x]].op == I_LD_ADV) return hoist_regs;
        }
        return 0;
    };
    auto flush = [&]() {
        if (cur.terms.empty()) return;
        std::sort(cur.body.begin(), cur.body.end());
        std::sort(cur.loads.begin(), cur.loads.end());
        p.sw_clusters.push_back(cur);
        cur = Program::SweepCluster();
        cost = 0;
        std::fill(in_cluster.begin(), in_cluster.end(), 0);
    };
    for (int pass = 0; pass < 2; ++pass) {                   // the per-point clusters first, then the affine ones
    flush();
    for (size_t ti = 0; ti < p.sw_terms.size(); ++ti) {
        if ((int)term_linear[ti] != pass) continue;
        cur.linear = pass == 1;
        const auto &t = p.sw_terms[ti];
        if (t.node < 0) { cur.terms.push_back((int)ti); continue; }
        std::vector<char> seen(nv, 0);
        std::vector<int> body, loads;
        B.collect(t.node, seen, body, loads);
        int extra = 0;
        for (int v : loads) if (!in_cluster[v]) extra += load_cost(v);
        extra += hoist_cost(t.node);
        if (!cur.terms.empty() && cost + extra > SWEEP_LOAD_BUDGET) flush();
        for (int v : loads) if (!in_cluster[v]) { in_cluster[v] = 1; cur.loads.push_back(v); cost += load_cost(v); }
        for (int v : body) if (!in_cluster[v]) { in_cluster[v] = 1; cur.body.push_back(v); }
        cost += hoist_cost(t.node);
        cur.linear = pass == 1;
        cur.terms.push_back((int)ti);
    }
    }
    flush();
    p.sweep_ok = !p.sw_clusters.empty();
}

}  // namespace

// bound (in units of p) to which the partner of a hoisted affine factor is prepared -- see the arithmetic where it is used
static constexpr double HOIST_PARTNER_BOUND = 8.0;

// the sweep form as C++ (see the comment on the signature below)
std::string emit_sweep_source(const Program &p, const std::string &name, bool shared_mul) {
    std::string o;
    if (!p.sweep_ok) return o;
    // shared_mul: one multiplier body per kernel (mul29_ni / sqr29_ni, rowprog_dev.cuh) -- the run-time compiled form, see emit_spec_source
    const std::string MUL = shared_mul ? "mul29_ni<F>(" : "G::mul(", SQR = shared_mul ? "sqr29_ni<F>(" : "G::sqr(";
    std::vector<int> def;
    {
        int nv = 0;
        for (auto &in : p.vins) nv = std::max(nv, in.dst + 1);
        def.assign(nv, -1);
        for (size_t i = 0; i < p.vins.size(); ++i) def[p.vins[i].dst] = (int)i;
    }
    auto S = [](int x) { return std::to_string(x); };
    // uniform entries the bodies need in a re-scaled form are added by plan_sweep only for coefficients; an addition of a
    // row value of level l and a uniform value is emitted with a run-time multiplication-free trick: the uniform operand is
    // multiplied by the level-raising constant like any other lower-level operand (rare: constants inside products).
    // NAME(C, row, npts, Uall, nu, acc, accumulate): adds (accumulate) or stores the LAZY 9 x 29-bit sum P(pt) * 2^256 + small
    // multiples of p into the thread's limb-planar LDS accumulators (sw_load / sw_store, rowprog_dev.cuh); NAME_one<F>() = the
    // uniform index of 2^261 mod p, with which the caller folds (sw_fold) and finishes (sw_finish) them.
    o += "template <class F> __device__ constexpr uint32_t " + name + "_one() { return " + S(p.sw_one) + "u; }\n";
    o += "template <class F>\n__device__ __forceinline__ void " + name +
         "(const RowCtx &C, uint32_t row, uint32_t npts, const fe_t *__restrict__ Uall, uint32_t nu, uint32_t *__restrict__ acc, bool accumulate) {\n";
    o += "    using G = Fp29<typename F::Params>;\n    const uint32_t mask = C.rows - 1; (void)mask;\n";
    bool first = true;
    double acc_bound = 2.0;                                      // an accumulator handed in by the caller is folded: < 2p
    // number of advice leaves of a product chain (the affine clusters hold nothing else)
    std::function<int(int)> chain = [&](int v) -> int {
        if (v < 0) return 0;
        const VInsn &in = p.vins[def[v]];
        if (in.op == I_LD_ADV) return 1;
        if (in.op == I_LD_SEL || in.op == I_LD_FIX) return 0;
        return chain(in.a) + chain(in.b);
    };
    for (size_t ci = 0; ci < p.sw_clusters.size(); ++ci) {
        const auto &cl = p.sw_clusters[ci];
        o += std::string("    {   // cluster ") + S((int)ci) + (cl.linear ? " (affine in the point)\n" : "\n");
        for (int v : cl.loads) {
            const VInsn &in = p.vins[def[v]];
            const std::string rr = "(row + " + std::to_string((uint32_t)in.b) + "u) & mask";
            if (in.op == I_LD_SEL) o += "        const fe_t l" + S(v) + " = ld_sel<F>(C, " + S(in.a) + ", " + rr + ");\n";
            else if (in.op == I_LD_FIX) o += "        const fe_t l" + S(v) + " = ld_fix<F>(C, " + S(in.a) + ", " + rr + ");\n";
            else o += "        fe_t l" + S(v) + ", s" + S(v) + "; adv_affine<F>(C, " + S(in.a) + ", " + rr + ", l" + S(v) + ", s" + S(v) + ");\n";
        }
        std::vector<char> is_load(def.size(), 0);            // column values are unpacked where they are used: a 9-limb copy of
        for (int v : cl.loads) is_load[v] = 1;               // every hoisted column, live across the loop body, spills
        // Hoisted affine factors (per-point clusters): q * (s * y) with q a fixed / selector column and s an advice leaf is computed as
        // (q s) * y, and q s is affine in the point -- its value and step cost two products per row, every point one lazy addition
        // instead of a product.  (The MainGate's q_5 s^5 terms: 3 instead of 4 products per state and point.)
        struct Hoist { int v, a, b, c, u; };
        std::vector<Hoist> hoists;
        std::map<int, size_t> hoist_of;                       // v -> index
        std::vector<char> hoisted_inner(def.size(), 0);
        if (!cl.linear) {
            std::vector<int> uses(def.size(), 0);
            for (int v : cl.body) {
                const VInsn &in = p.vins[def[v]];
                if (in.a >= 0) ++uses[in.a];
                if (in.op <= I_MUL && in.b >= 0) ++uses[in.b];
            }
            for (int ti : cl.terms) if (p.sw_terms[ti].node >= 0) ++uses[p.sw_terms[ti].node];
            auto fixed_leaf = [&](int x) { return x >= 0 && is_load[x] && p.vins[def[x]].op != I_LD_ADV; };
            auto adv_leaf = [&](int x) { return x >= 0 && is_load[x] && p.vins[def[x]].op == I_LD_ADV; };
            for (int v : cl.body) {
                const VInsn &in = p.vins[def[v]];
                if (in.op != I_MUL) continue;
                for (int o1 = 0; o1 < 2 && !hoist_of.count(v); ++o1) {
                    const int a = o1 ? in.b : in.a, u = o1 ? in.a : in.b;
                    if (!fixed_leaf(a) || u < 0 || is_load[u] || p.vins[def[u]].op != I_MUL || uses[u] != 1 || hoisted_inner[u]) continue;
                    const VInsn &iu = p.vins[def[u]];
                    for (int o2 = 0; o2 < 2; ++o2) {
                        const int b = o2 ? iu.b : iu.a, c = o2 ? iu.a : iu.b;
                        if (!adv_leaf(b) || c == b) continue;
                        hoist_of[v] = hoists.size();
                        hoists.push_back({v, a, b, c, u});
                        hoisted_inner[u] = 1;
                        break;
                    }
                }
            }
        }
        // One evaluation of the cluster's terms.  IN: indentation; X: name prefix of the temporaries; slope: the advice leaves
        // enter with their STEP and the terms without an advice leaf are left out (affine clusters).  -> expression of the lazy
        // sum and its bound in units of p (empty: nothing to add).
        auto gen = [&](const std::string &IN, const std::string &X, bool slope, double &total_b) -> std::string {
        std::map<int, double> bound;                           // static bound of a value in units of p (normalised limbs)
        for (int v : cl.loads) bound[v] = 1.0;
        auto bnd = [&](int x) { return x >= 0 ? bound[x] : 1.0; };
        auto lvl = [&](int x) { return x >= 0 ? p.sw_level[x] : 0; };
        int tmp = 0;
        const std::string D = IN + "const f29_t ";
        // operand x at `level` with a bound <= max_bound: the expression text; b_out = its bound
        auto prep = [&](int x, int level, double max_bound, double &b_out) -> std::string {
            if (x < 0) {                                         // row-independent operand: the host keeps a copy at every level needed
                b_out = 1.0;
                const int u = -x - 1;
                if (level <= 0) return "G::unpack(U[" + S(u) + "])";
                auto it = p.sw_uat.find({u, level});
                return "G::unpack(U[" + S(it == p.sw_uat.end() ? u : it->second) + "])";
            }
            std::string e;
            if (is_load[x]) e = std::string("G::unpack(") + ((slope && p.vins[def[x]].op == I_LD_ADV) ? "s" : "l") + S(x) + ")";
            else e = X + "x" + S(x);
            double b = bnd(x);
            if (lvl(x) < level) {                                // product with the raw constant 2^(261 - 5 delta): + delta levels
                const std::string t = X + "r" + S(tmp++);
                o += D + t + " = " + MUL + e + ", G::unpack(U[" + S(p.sw_raise[level - lvl(x)]) + "]));\n";
                e = t;
                b = 2.0;
            }
            if (b > max_bound) {                                 // product with 2^261 mod p: the same value, below 2p again
                const std::string t = X + "r" + S(tmp++);
                o += D + t + " = " + MUL + e + ", G::unpack(U[" + S(p.sw_one) + "]));\n";
                e = t;
                b = 2.0;
            }
            b_out = b;
            return e;
        };
        // in slope mode only the values the degree-1 terms need are computed
        std::vector<char> want(def.size(), 1);
        if (slope) {
            std::fill(want.begin(), want.end(), 0);
            std::function<void(int)> mark = [&](int v) {
                if (v < 0 || want[v]) return;
                want[v] = 1;
                const VInsn &in = p.vins[def[v]];
                if (in.op > I_LD_ADV) { mark(in.a); if (in.op <= I_MUL) mark(in.b); }
            };
            for (int ti : cl.terms) {
                const auto &t = p.sw_terms[ti];
                if (t.node >= 0 && chain(t.node) == 1) mark(t.node);
            }
        }
        for (int v : cl.body) {
            if (!want[v] || hoisted_inner[v]) continue;
            const VInsn &in = p.vins[def[v]];
            const std::string d = D + X + "x" + S(v) + " = ";
            double ba, bb;
            if (hoist_of.count(v)) {                             // (q s) * y with the affine factor kept in `aff`
                const Hoist &h = hoists[hoist_of[v]];
                // `aff` is a product (< 2p) plus one step (< 2p) per point passed: < 2p (1 + pt) at point pt, and the sweep form takes
                // at most DMAX + 1 points -- budgeted as 2p (1 + DMAX + 1) = 20p.  mul needs A * B < (2^261 / p) p^2 = 169.2 p^2 (both
                // fields), so the partner is prepared to <= 8p: 20 * 8 = 160.  (The general operand bound 12 gives 240: a partner that
                // is a sum of 9 .. 12 column values broke the multiplier's stated precondition.)
                static_assert(2.0 * (1 + DMAX + 1) * HOIST_PARTNER_BOUND < 165.0, "hoisted factor * partner must stay below 2^261 / p");
                std::string c = prep(h.c, lvl(h.c), HOIST_PARTNER_BOUND, bb);
                o += d + MUL + "aff" + S(v) + ", " + c + ");\n";
                bound[v] = 2.0;
                continue;
            }
            switch (in.op) {
            case I_MUL: {
                std::string a = prep(in.a, lvl(in.a), 12.0, ba), b = prep(in.b, lvl(in.b), 12.0, bb);      // a uniform operand enters at level 0
                o += d + MUL + a + ", " + b + ");\n";
                bound[v] = 2.0;
                break;
            }
            case I_SQR: {
                std::string a = prep(in.a, lvl(in.a), 12.0, ba);
                o += d + SQR + a + ");\n";
                bound[v] = 2.0;
                break;
            }
            case I_ADD: {
                const int L = p.sw_level[v];
                std::string a = prep(in.a, L, 30.0, ba), b = prep(in.b, L, 30.0, bb);
                o += d + "G::normalize(G::add_lazy(" + a + ", " + b + "));\n";
                bound[v] = ba + bb;
                break;
            }
            case I_SUB: {
                const int L = p.sw_level[v];
                std::string a = prep(in.a, L, 30.0, ba), b = prep(in.b, L, 30.0, bb);
                const int cp = (int)bb + 1;
                o += d + "G::normalize(G::template sub_lazy<" + S(cp) + ", 0>(" + a + ", " + b + "));\n";
                bound[v] = ba + cp;
                break;
            }
            case I_DBL: {
                std::string a = prep(in.a, lvl(in.a), 30.0, ba);
                o += d + "G::normalize(G::add_lazy(" + a + ", " + a + "));\n";
                bound[v] = 2 * ba;
                break;
            }
            default: {
                std::string a = prep(in.a, lvl(in.a), 30.0, ba);
                const int cp = (int)ba + 1;
                o += d + "G::normalize(G::template neg_lazy<" + S(cp) + ", 0>(" + a + "));\n";
                bound[v] = cp;
                break;
            }
            }
        }
        // the terms: terms sharing a coefficient are summed first, then ONE closing product with the pre-scaled coefficient per
        // group -> ABI form; everything stays lazy (sums of values < 2p, normalised limbs) down to the accumulator in LDS
        std::vector<int> order;                                  // coefficient groups in first-appearance order
        std::map<int, std::vector<int>> groups;
        for (int ti : cl.terms) {
            const auto &t = p.sw_terms[ti];
            if (slope && (t.node < 0 || chain(t.node) != 1)) continue;
            if (!groups.count(t.coef)) order.push_back(t.coef);
            groups[t.coef].push_back(ti);
        }
        std::string total;
        total_b = 0;
        auto lazy_add = [&](std::string &sum, double &b, const std::string &e, double be, bool minus) {
            const std::string r = X + "r" + S(tmp++);
            if (sum.empty()) {
                if (minus) {
                    const int cp = (int)be + 1;
                    o += D + r + " = G::normalize(G::template neg_lazy<" + S(cp) + ", 0>(" + e + "));\n";
                    b = cp;
                } else {
                    sum = e;
                    b = be;
                    return;
                }
            } else if (minus) {
                const int cp = (int)be + 1;
                o += D + r + " = G::normalize(G::template sub_lazy<" + S(cp) + ", 0>(" + sum + ", " + e + "));\n";
                b += cp;
            } else {
                o += D + r + " = G::normalize(G::add_lazy(" + sum + ", " + e + "));\n";
                b += be;
            }
            sum = r;
        };
        auto fold = [&](std::string &sum, double &b, double limit) {
            if (b <= limit) return;
            const std::string r = X + "r" + S(tmp++);
            o += D + r + " = " + MUL + sum + ", G::unpack(U[" + S(p.sw_one) + "]));\n";
            sum = r;
            b = 2.0;
        };
        for (int key : order) {
            const auto &g = groups[key];
            const auto &t0 = p.sw_terms[g[0]];
            std::string val;
            bool negate = t0.sign < 0;                           // the group enters the cluster sum as +-(first +- ...)
            double vb = 1.0;
            if (t0.node < 0) {
                val = "G::unpack(U[" + S(t0.coef) + "])";        // constant term (ABI form, canonical)
            } else {
                // all terms of a group share the coefficient, hence the level (the scale 2^(5 (level + 1)) is part of the entry)
                std::string sum;
                double b = 0;
                for (size_t j = 0; j < g.size(); ++j) {
                    const auto &t = p.sw_terms[g[j]];
                    double bj;
                    std::string e = prep(t.node, lvl(t.node), 12.0, bj);
                    lazy_add(sum, b, e, bj, (t.sign < 0) != negate);
                    fold(sum, b, 12.0);
                }
                const std::string r = X + "r" + S(tmp++);
                o += D + r + " = " + MUL + sum + ", G::unpack(U[" + S(t0.coef) + "]));\n";
                val = r;
                vb = 2.0;
            }
            lazy_add(total, total_b, val, vb, negate);
            fold(total, total_b, 24.0);
        }
        if (!total.empty() && slope) fold(total, total_b, 2.0);          // the step is added once per point: keep it below 2p
        return total;
        };   // gen

        if (!cl.linear) {
            for (const Hoist &h : hoists) {
                o += "        f29_t aff" + S(h.v) + " = " + MUL + "G::unpack(l" + S(h.a) + "), G::unpack(l" + S(h.b) + "));\n";
                o += "        const f29_t affs" + S(h.v) + " = npts > 1 ? " + MUL + "G::unpack(l" + S(h.a) + "), G::unpack(s" + S(h.b) + ")) : aff" + S(h.v) + ";\n";
            }
            o += "        for (uint32_t pt = 0; pt < npts; ++pt) {\n";
            o += "            const fe_t *__restrict__ U = Uall + (size_t)pt * nu; (void)U;\n";
            double total_b = 0;
            const std::string total = gen("            ", "", false, total_b);
            if (first) {
                o += "            sw_store(acc, pt, accumulate ? G::normalize(G::add_lazy(sw_load(acc, pt), " + total + ")) : " + total + ");\n";
            } else {
                o += "            sw_store(acc, pt, G::normalize(G::add_lazy(sw_load(acc, pt), " + total + ")));\n";
            }
            acc_bound += total_b;
            if (acc_bound > 100.0) {                                 // fold the accumulators before they outgrow the 261-bit limbs
                o += "            sw_store(acc, pt, " + MUL + "sw_load(acc, pt), G::unpack(U[" + S(p.sw_one) + "])));\n";
                acc_bound = 2.0;
            }
            for (int v : cl.loads)
                if (p.vins[def[v]].op == I_LD_ADV) o += "            l" + S(v) + " = F::add(l" + S(v) + ", s" + S(v) + ");\n";
            for (const Hoist &h : hoists)                         // < 2p (1 + points) <= 20p; its partner is prepared to HOIST_PARTNER_BOUND (gen)
                o += "            aff" + S(h.v) + " = G::normalize(G::add_lazy(aff" + S(h.v) + ", affs" + S(h.v) + "));\n";
            o += "        }\n    }\n";
        } else {
            // value at the first point + slope, then one lazy addition per further point (coefficients do not depend on the point)
            o += "        const fe_t *__restrict__ U = Uall; (void)U;\n";
            double vb = 0, sb = 0;
            std::string val = gen("        ", "v", false, vb);
            const std::string step = gen("        ", "d", true, sb);
            if (val.empty()) { val = "G::unpack(F::zero())"; vb = 1.0; }
            if (vb > 2.0) {
                o += "        const f29_t vfold = " + MUL + val + ", G::unpack(U[" + S(p.sw_one) + "]));\n";
                val = "vfold";
                vb = 2.0;
            }
            o += "        f29_t cur = " + val + ";\n";
            o += "        for (uint32_t pt = 0; pt < npts; ++pt) {\n";
            if (first) o += "            sw_store(acc, pt, accumulate ? G::normalize(G::add_lazy(sw_load(acc, pt), cur)) : cur);\n";
            else o += "            sw_store(acc, pt, G::normalize(G::add_lazy(sw_load(acc, pt), cur)));\n";
            if (!step.empty()) o += "            cur = G::normalize(G::add_lazy(cur, " + step + "));\n";
            const double worst = vb + (step.empty() ? 0.0 : sb * (double)DMAX);      // cur at the last of <= DMAX + 1 points
            acc_bound += worst;
            if (acc_bound > 100.0) {
                o += "            sw_store(acc, pt, " + MUL + "sw_load(acc, pt), G::unpack(U[" + S(p.sw_one) + "])));\n";
                acc_bound = 2.0;
            }
            o += "        }\n    }\n";
        }
        first = false;
    }
    o += "}\n";
    return o;
}

namespace {

static bool build_program(const Ast &ast, int root, const FieldOps &f, const Ctx &ctx, bool fold_mode, Program &p,
                          std::string &err) {
    Compiler c(ast, f, ctx, fold_mode);
    Val v = c.walk(root);
    if (!c.err.empty()) { err = c.err; return false; }
    int result_vreg = -1;
    uint32_t result_uniform = 0;
    if (v.cls == 2) result_vreg = v.id; else result_uniform = UNIFORM_BIT | (uint32_t)c.as_uniform(v);
    p.uops = c.uops;
    allocate(c.vins, c.nvreg, result_vreg, p.insns, p.result, p.nslots);
    if (result_vreg < 0) p.result = result_uniform;
    p.vins = c.vins;
    p.result_vreg = result_vreg;
    p.fingerprint = fingerprint_of(p);
    plan_sweep(p, f);               // appends coefficient entries to p.uops (the fingerprint above is that of the plain program)
    return true;
}

}  // namespace

// inverse Vandermonde for the nodes first .. first + d, all rows: out[k * (d + 1) + j] = coefficient of X^k in L_j(X), k = 0..d
std::vector<fe_t> inverse_vandermonde_at(const FieldOps &f, size_t d, uint64_t first) {
    const size_t m = d + 1;
    std::vector<fe_t> out(m * m);
    for (size_t j = 0; j < m; ++j) {
        std::vector<fe_t> poly(1, f.one());        // prod_{t != j} (X - x_t)
        fe_t denom = f.one();
        for (size_t t = 0; t < m; ++t) {
            if (t == j) continue;
            const fe_t ft = f.from_u64(first + t);
            std::vector<fe_t> nx(poly.size() + 1, f.zero());
            for (size_t i = 0; i < poly.size(); ++i) {
                nx[i + 1] = f.add(nx[i + 1], poly[i]);
                nx[i] = f.sub(nx[i], f.mul(poly[i], ft));
            }
            poly.swap(nx);
            denom = f.mul(denom, f.sub(f.from_u64(first + j), ft));
        }
        const fe_t di = f.inv(denom);
        for (size_t k = 0; k <= d; ++k) out[k * m + j] = f.mul(poly[k], di);
    }
    return out;
}

bool compile_structure(int field, size_t num_selectors, size_t num_fixed, size_t num_advice,
                       const uint64_t *gates, size_t gates_words, size_t num_gates, size_t num_lookups, bool has_vector_lookup,
                       const uint64_t *lookup_exprs, size_t lookup_words, Compiled &out, int &rc, std::string &err) {
    rc = 4;
    FieldOps f{field};
    Ast ast;
    std::vector<int> roots, lroots;
    if (!parse_gates(gates, gates_words, num_gates, ast, roots, err)) return false;
    if (num_lookups && !parse_gates(lookup_exprs, lookup_words, 2 * num_lookups, ast, lroots, err)) return false;
    if (!num_lookups && has_vector_lookup) { err = "has_vector_lookup without lookups"; return false; }
    int32_t min_rot = 0, max_rot = 0;
    for (const Node &nd : ast.n)
        if (nd.kind == N_POLY) { min_rot = std::min(min_rot, nd.rot); max_rot = std::max(max_rot, nd.rot); }
    if (num_selectors + num_fixed == 0) { err = "Fixed & Selectors can't be empty in one time"; return false; }   // eval.rs:47-54
    out.min_rot = min_rot;
    out.max_rot = max_rot;
    // ConstraintSystemMetainfo::build: the gate-compression challenge comes after the lookup challenges
    // (r1 [, r2]), i.e. ctx.num_challenges starts at 2 / 1 / 0
    // (src/table/constraint_system_metainfo.rs:81-97) -> CompressedGates::new (src/plonk/mod.rs:84-107)
    Ctx ctx{num_selectors, num_fixed, num_advice, has_vector_lookup ? (size_t)2 : (num_lookups ? (size_t)1 : (size_t)0)};
    ctx.num_lookups = num_lookups;
    int compressed = compress(ast, roots, ctx.num_challenges, f);
    ctx.num_challenges = num_challenges(ast, compressed);
    out.s_num_challenges = ctx.num_challenges;
    int homog;
    size_t degree;
    if (!homogeneous(ast, compressed, ctx, homog, degree, err)) { rc = 7; return false; }
    out.h_num_challenges = num_challenges(ast, homog);
    out.degree = degree;
    if (degree > DEGREE_LIMIT) { err = "folding degree " + std::to_string(degree) + " exceeds the supported maximum 255"; return false; }
    if (!build_program(ast, homog, f, ctx, true, out.cross, err) ||
        !build_program(ast, compressed, f, ctx, false, out.plain_compressed, err) ||
        !build_program(ast, homog, f, ctx, false, out.plain_homogeneous, err)) {
        rc = 7;
        return false;
    }
    if (degree) out.vinv = inverse_vandermonde_rows(f, degree);
    out.gate_progs.resize(roots.size());
    for (size_t g = 0; g < roots.size(); ++g) {
        if (!build_program(ast, roots[g], f, ctx, false, out.gate_progs[g], err)) { rc = 7; return false; }
        out.max_gate_degree = std::max(out.max_gate_degree, expr_degree(ast, roots[g], ctx));
    }
    if (field == 0 && out.max_gate_degree >= 1 && out.max_gate_degree <= 64) {     // 6 inversions each: once per structure, not per prove
        out.vinv_g = inverse_vandermonde_rows(f, out.max_gate_degree);
        out.vinv_g1 = inverse_vandermonde_at(f, out.max_gate_degree, 1);
    }
    // lookup / table polynomials see the advice COLUMNS only (LookupEvalDomain, src/plonk/eval.rs:106-134)
    {
        Ctx lctx{num_selectors, num_fixed, num_advice, 0};
        out.lookup_progs.resize(lroots.size());
        for (size_t i = 0; i < lroots.size(); ++i)
            if (!build_program(ast, lroots[i], f, lctx, false, out.lookup_progs[i], err)) { rc = 7; return false; }
    }
    return true;
}

// evaluate the uniform program for one point: challenge i -> ch[i] + pt * ch[i + fold_offset]
bool eval_uniform(const Program &p, const FieldOps &f, const fe_t *ch, size_t n_ch, size_t fold_offset, bool fold,
                  uint32_t pt, fe_t *out, std::string &err) {
    fe_t fpt = f.from_u64(pt);
    for (size_t i = 0; i < p.uops.size(); ++i) {
        const UOp &u = p.uops[i];
        switch (u.op) {
        case 0: out[i] = u.c; break;
        case 1: {
            size_t a = (size_t)u.chal;
            if (a >= n_ch) { err = "challenge index " + std::to_string(a) + " out of boundary " + std::to_string(n_ch); return false; }
            out[i] = ch[a];
            if (fold) {
                size_t b = a + fold_offset;
                if (b >= n_ch) { err = "challenge index " + std::to_string(b) + " out of boundary " + std::to_string(n_ch); return false; }
                if (pt) out[i] = f.add(out[i], f.mul(fpt, ch[b]));
            }
            break;
        }
        case 2: out[i] = f.add(out[u.a], out[u.b]); break;
        case 3: out[i] = f.sub(out[u.a], out[u.b]); break;
        case 4: out[i] = f.mul(out[u.a], out[u.b]); break;
        case 6: {                                     // u[a] * 2^(5 b): operands of the 2^261-radix multiplier (sweep form)
            fe_t x = out[u.a];
            for (int k = 0; k < 5 * (u.b < 0 ? -u.b : u.b); ++k) x = u.b < 0 ? f.halve(x) : f.add(x, x);
            out[i] = x;
            break;
        }
        default: out[i] = f.neg(out[u.a]); break;
        }
    }
    return true;
}

}  // namespace rowprog
}  // namespace srs
