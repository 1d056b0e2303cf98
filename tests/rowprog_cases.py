"""The row-program compiler's output, pinned: tests/golden/rowprog_programs.json holds a set of structures AS DATA (field, column
counts, gate and lookup expressions in the tuple form of sirius_amd.expression, as nested lists) and, for each, what the library
derived from them -- num_challenges, the folding degree and, for every `which` srs_structure_program_source accepts (0 cross terms,
1 compressed, 2 homogeneous, 3 + g the gates one by one), the fingerprint, the ahead-of-time kernel id with the run-time compiler
off, and the byte length and SHA-256 of the emitted source (straight-line + sweep form).

`measure` rebuilds one structure on the loaded library (CPU emulator or the real one) and returns the same fields; the tests
compare them with the file.  The compiler does not look at the rows: every structure has 2^3 rows of zero columns.

Re-recording (only when the emitted programs are MEANT to change): make -C tests/emu && python tests/rowprog_cases.py"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "rowprog_programs.json")
K = 3


def load():
    with open(PATH) as f:
        return json.load(f)["structures"]


def measure(S, e):
    """the recorded fields of structure `e` (an entry of the file; only its inputs are read) on the library `S` runs on"""
    from sirius_amd import _lib
    lib = _lib.lib()
    rows = 1 << K
    sels = [np.zeros(rows, np.uint8) for _ in range(e["num_selectors"])]
    fixed = [np.zeros((rows, 4), np.uint64) for _ in range(e["num_fixed"])]
    lookups = [(inp, tab) for inp, tab in e["lookups"]] if e["lookups"] else None
    with S.tuning(no_jit=1):
        St = S.PlonkStructure(e["field"], K, sels, fixed, e["num_advice"], e["gates"], lookups=lookups)
    out = {"num_challenges": St.num_challenges, "degree": St.num_cross_terms, "programs": []}
    for which in [0, 1, 2] + [3 + g for g in range(len(St.gates))]:
        fp, sid = C.c_uint64(), C.c_int()
        n = lib.srs_structure_program_source(St._h, which, None, 0, C.byref(fp), C.byref(sid))
        buf = C.create_string_buffer(n + 1)
        assert lib.srs_structure_program_source(St._h, which, buf, n + 1, None, None) == n
        out["programs"].append({"which": which, "fingerprint": f"0x{fp.value:016x}", "spec_id": sid.value, "bytes": n,
                                "sha256": hashlib.sha256(buf.raw[:n]).hexdigest()})
    St.close()
    return out


def check(S):
    """every structure of the file, rebuilt on `S`'s library, gives every recorded field"""
    entries = load()
    assert len(entries) == 15
    for e in entries:
        got = measure(S, e)
        for key in ("num_challenges", "degree"):
            assert got[key] == e[key], (e["name"], key, got[key], e[key])
        assert len(got["programs"]) == len(e["programs"]), e["name"]
        for g, w in zip(got["programs"], e["programs"]):
            assert g == w, (e["name"], g, w)


def _inputs():
    """the structures to record (needs the oracle: the random circuits are filtered by their folding degree as the test that
    accepts them does)"""
    import random
    import sirius_amd as S
    from sirius_amd.workloads import gates_for
    from oracle import expr as OE
    from lookup_cases import _shape, _to_product_expr
    from test_emu_jit import _random_expr
    X = S.expression
    out = []

    def add(name, field, nsel, nfix, nadv, gates, lookups=None):
        out.append({"name": name, "field": field, "num_selectors": nsel, "num_fixed": nfix, "num_advice": nadv, "gates": gates, "lookups": lookups})
    for field, gate_T in [(0, [5, 3]), (0, [5]), (1, [3, 2]), (0, [2, 5, 2])]:
        gates, nfix, nadv = gates_for(gate_T)
        add("main_gates_" + "_".join(map(str, gate_T)), field, 0, nfix, nadv, gates)
    for variant in ("vector", "two"):                       # tests/lookup_cases.py
        ns, nf, na, ogates, olookups = _shape(variant)
        add("lookup_" + variant, 0, ns, nf, na, [_to_product_expr(X, g) for g in ogates],
            [([_to_product_expr(X, x) for x in i], [_to_product_expr(X, x) for x in t]) for i, t in olookups])
    rnd = random.Random(2029)                               # the eight circuits test_emu_jit_random_circuits accepts
    done = attempts = 0
    while done < 8 and attempts < 400:
        attempts += 1
        nsel, nfix, nadv = rnd.choice([0, 1]), rnd.randrange(1, 4), rnd.randrange(1, 4)
        gates = [_random_expr(rnd, nsel, nfix, nadv, rnd.randrange(2, 5)) for _ in range(rnd.choice([1, 1, 2]))]
        try:
            degs = [OE.homogeneous(g, OE.QueryIndexContext(nsel, nfix, nadv, 0, 0))[1] for g in gates]
        except Exception:
            continue
        if not all(2 <= d <= 6 for d in degs):
            continue
        add(f"random_{attempts}", rnd.choice([0, 1]), nsel, nfix, nadv, gates)
        done += 1
    assert done == 8
    from test_sangria_gpu import _high_degree_gates         # the structure test_emu_high_folding_degree builds
    add("high_degree_10", 0, 0, 10, 3, _high_degree_gates(X, 10))
    return json.loads(json.dumps(out))                      # tuples -> lists, as the tests will read them


def main():
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import sirius_amd as S
    from sirius_amd import _lib
    _lib.load(os.path.join(ROOT, "tests", "emu", "libsirius_emu.so"))
    entries = _inputs()
    for e in entries:
        e.update(measure(S, e))
    with open(PATH, "w") as f:
        f.write('{"k": %d, "structures": [\n' % K + ",\n".join(json.dumps(e, separators=(",", ":")) for e in entries) + "\n]}\n")
    print("wrote", PATH, len(entries), "structures,", sum(len(e["programs"]) for e in entries), "programs")


if __name__ == "__main__":
    main()
