// How long does hiprtc take over a gate set's ProtoGalaxy leaf unit, next to the structure's cross-term unit?  Host only (no device):
// the row-program compiler, the unit emitters and jit::compile_only of the library itself, on gate sets serialised by
// tools/pg_jit_compile_probe.py.  The record behind PG_JIT_MAX_INSNS (csrc/rowprog.hip): profiles/pg_leaves_jit_ab.txt.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -Isirius_amd/csrc tools/pg_jit_compile_probe.cpp -o tools/pg_jit_compile_probe \
//         -Lsirius_amd/csrc -lsirius_amd -Wl,-rpath,$PWD/sirius_amd/csrc
//   python tools/pg_jit_compile_probe.py            (writes the gate sets, runs this program on each)
// file: u64 field, num_selectors, num_fixed, num_advice, num_gates, n_words, then the words of serialize_gates
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rowprog.h"
#include "rowprog_compile.h"

using namespace srs;

static double timed_compile(const std::string &src, size_t &bytes, std::string &log) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = jit::compile_only(src, &bytes, log);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return ok ? s : -1.0;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        FILE *f = std::fopen(argv[i], "rb");
        uint64_t h[6];
        if (!f || std::fread(h, 8, 6, f) != 6) { std::printf("%s: cannot read\n", argv[i]); return 1; }
        std::vector<uint64_t> words(h[5]);
        if (std::fread(words.data(), 8, words.size(), f) != words.size()) { std::printf("%s: short file\n", argv[i]); return 1; }
        std::fclose(f);
        rowprog::Compiled c;
        int rc = 0;
        std::string err;
        if (!rowprog::compile_structure((int)h[0], h[1], h[2], h[3], words.data(), words.size(), h[4], 0, false, nullptr, 0, c, rc, err)) {
            std::printf("%s: compile_structure rc %d: %s\n", argv[i], rc, err.c_str());
            return 1;
        }
        bool sweep = false;
        const std::string leaf = rowprog::pg_leaf_unit_source(c, &sweep), cross = rowprog::cross_unit_source(c, (int)h[0]);
        if (const char *dump = std::getenv("PG_JIT_PROBE_DUMP")) {      // keep the leaf unit: hipcc --cuda-device-only + llvm-readelf --notes give its resources
            if (FILE *o = std::fopen((std::string(dump) + "/leaf_unit_" + std::to_string(i) + ".hip").c_str(), "wb")) { std::fwrite(leaf.data(), 1, leaf.size(), o); std::fclose(o); }
        }
        size_t lb = 0, cb = 0;
        std::string log;
        const double ls = timed_compile(leaf, lb, log);
        if (ls < 0) std::printf("leaf unit failed: %.2000s\n", log.c_str());
        const double cs = c.degree <= rowprog::DMAX ? timed_compile(cross, cb, log) : 0.0;
        std::printf("%-28s gates %2zu  leaf insns %5zu  sweep %d  leaf unit %7zu B source %7.2f s %8zu B code | cross degree %2zu insns %5zu  %7.2f s %8zu B code | ratio %.1f\n",
                    argv[i], c.gate_progs.size(), rowprog::pg_leaf_unit_insns(c), (int)sweep, leaf.size(), ls, lb, c.degree, c.cross.vins.size(), cs, cb,
                    cs > 0 ? ls / cs : 0.0);
        std::fflush(stdout);
    }
    return 0;
}
