"""Serialises the gate sets whose ProtoGalaxy leaf units are timed under hiprtc and runs tools/pg_jit_compile_probe on them (host only, no
device; build line in tools/pg_jit_compile_probe.cpp).  The record: profiles/pg_leaves_jit_ab.txt.
usage: python tools/pg_jit_compile_probe.py [directory for the gate-set files; default: a temporary one]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gate_sets():
    from sirius_amd.workloads import gates_for, high_degree_gate
    out = {}
    for name, gate_T in (("main_2", [2]), ("main_5_3", [5, 3]), ("main_2_3_x8", [2, 3] * 8), ("main_5_x4", [5] * 4)):
        out[name] = gates_for(gate_T)
    gates, nfix, nadv = gates_for([5, 3])
    for d in (9, 15):
        out[f"degree{d}_5_3"] = ([high_degree_gate(5, d, 0, 0, 0, nfix), gates[1]], nfix, nadv)      # bench.py --full: the degree-15 pair
    return out


def main():
    from sirius_amd.expression import serialize_gates
    where = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="pg_jit_probe_")
    files = []
    for name, (gates, nfix, nadv) in gate_sets().items():
        words = np.ascontiguousarray(serialize_gates(list(gates), 0), dtype=np.uint64)
        path = os.path.join(where, name + ".gates")
        with open(path, "wb") as f:
            f.write(np.array([0, 0, nfix, nadv, len(gates), len(words)], dtype=np.uint64).tobytes())
            f.write(words.tobytes())
        files.append(path)
    subprocess.check_call([os.path.join(ROOT, "tools", "pg_jit_compile_probe")] + files)


if __name__ == "__main__":
    main()
