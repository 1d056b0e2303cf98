// jit_emu_units.h -- TEST INFRASTRUCTURE: the part of the run-time compilation interface (csrc/jit.h) that serves units with SEVERAL
// kernels -- compile_unit, entry, launch_grid -- for the CPU logic emulator; csrc/jit.h includes it under SRS_EMU only.  The single-kernel
// half (enabled, compile, compile_only, launch, release) stays in jit_emu.cpp.  This file REPEATS its g++ command, temporary-file
// scheme and audit drain (keep the two in step).  A unit is compiled with g++ against the emulator headers into a
// shared object; every kernel of the table below that the unit defines gets a launcher appended (the product never sees it):
//   srs_jit_launch_emu_<kernel>(blocks_x, blocks_y, threads, smem, args)
#pragma once
#include <dlfcn.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#ifdef SRS_F29_AUDIT
#include "field29_audit.h"
#endif

namespace srs {
namespace jit {
namespace emu_units {

// prefixes of their own: jit_emu.cpp numbers its files from 0 as well, and dlopen() finds a loaded object BY NAME (see there)
#ifdef SRS_F29_AUDIT
inline const char *prefix() { return "/tmp/srs_emu_audit_unit_"; }
inline const char *audit_flag() { return "-DSRS_F29_AUDIT -fno-gnu-unique "; }       // as the library itself (Makefile: AUDIT_FLAGS)
#else
inline const char *prefix() { return "/tmp/srs_emu_unit_"; }
inline const char *audit_flag() { return ""; }
#endif

// the kernels a unit may define and the argument block each takes by value (csrc/rowprog.hip: pg_leaf_unit)
struct Entry { const char *name, *args; };
inline const Entry *entries(size_t &n) {
    static const Entry k[] = {{"srs_pg_jit_leaves_run", "PgArgs"}, {"srs_pg_jit_leaves_sweep", "PgArgs"}, {"srs_pg_jit_F_leaves", "PgFArgs"}};
    n = sizeof(k) / sizeof(k[0]);
    return k;
}
inline void *launcher_symbol(void *module, const char *name) { return dlsym(module, (std::string("srs_jit_launch_emu_") + name).c_str()); }

}  // namespace emu_units

inline bool compile_unit(const std::string &source, const char *entry_name, Kernel &out, std::string &log) {
    static std::atomic<int> seq{0};
    const std::string base = emu_units::prefix() + std::to_string((long)getpid()) + "_" + std::to_string(seq++);
    const std::string src = base + ".cpp", errf = base + ".err", so = base + ".so";
    std::string unit = source;
    size_t n = 0;
    const emu_units::Entry *tab = emu_units::entries(n);
    for (size_t i = 0; i < n; ++i) {
        if (source.find(std::string(" ") + tab[i].name + "(") == std::string::npos) continue;
        unit += std::string("\nextern \"C\" void srs_jit_launch_emu_") + tab[i].name +
                "(unsigned blocks_x, unsigned blocks_y, unsigned threads, unsigned smem, const void *a) {\n    hipemu::launch(srs::rowprog::" + tab[i].name +
                ", dim3(blocks_x, blocks_y), dim3(threads), (size_t)smem, *static_cast<const srs::rowprog::" + tab[i].args + " *>(a));\n}\n";
    }
#ifdef SRS_F29_AUDIT
    // the unit is a shared object of its own with a violation table of its own: launch_grid drains it into the library's
    unit += "\nextern \"C\" void srs_jit_audit_drain_emu(unsigned long long *counts, char *sites) { srs::f29_audit::read_table(1, (uint64_t *)counts, sites); }\n";
#endif
    if (FILE *f = std::fopen(src.c_str(), "wb")) { std::fwrite(unit.data(), 1, unit.size(), f); std::fclose(f); }
    else { log = "cannot write " + src; return false; }
    const std::string cmd = std::string("g++ -std=c++20 -O1 -fPIC -DSRS_EMU -I" SRS_EMU_INC1 " -I" SRS_EMU_INC2 " -pthread -Wno-unknown-pragmas -Wno-attributes ") +
                            emu_units::audit_flag() + "-shared -o " + so + " " + src + " 2> " + errf;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = std::system(cmd.c_str());
    out.compile_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != 0) {
        log = "g++ failed: " + cmd + "\n";
        if (FILE *f = std::fopen(errf.c_str(), "rb")) {
            char buf[4096];
            size_t got = std::fread(buf, 1, sizeof buf - 1, f);
            buf[got] = 0;
            log += buf;
            std::fclose(f);
        }
    }
    if (!std::getenv("SRS_JIT_DUMP")) std::remove(src.c_str());
    std::remove(errf.c_str());
    if (rc != 0) return false;
    void *h = dlopen(so.c_str(), RTLD_NOW | RTLD_LOCAL);
    std::remove(so.c_str());                                 // the mapping stays
    if (!h) { log = std::string("dlopen: ") + dlerror(); return false; }
    void *fn = emu_units::launcher_symbol(h, entry_name);
    if (!fn) { log = std::string("entry point ") + entry_name + " not found in the compiled unit"; dlclose(h); return false; }
    out.module = h;
    out.function = fn;
    return true;
}

inline bool entry(const Kernel &owner, const char *name, Kernel &out, std::string &log) {
    void *fn = owner.module ? emu_units::launcher_symbol(owner.module, name) : nullptr;
    if (!fn) { log = std::string("entry point ") + name + " not found in the compiled module"; return false; }
    out.module = nullptr;
    out.function = fn;
    out.compile_seconds = 0;
    return true;
}

inline bool launch_grid(const Kernel &k, unsigned blocks_x, unsigned blocks_y, unsigned threads, unsigned smem_bytes, const void *arg_struct, hipStream_t) {
    if (!k.function) return false;
    reinterpret_cast<void (*)(unsigned, unsigned, unsigned, unsigned, const void *)>(k.function)(blocks_x, blocks_y, threads, smem_bytes, arg_struct);
#ifdef SRS_F29_AUDIT
    Dl_info where;                                           // the unit the launcher lives in (a kernel from entry() carries no module handle)
    void *unit = dladdr(k.function, &where) ? dlopen(where.dli_fname, RTLD_NOW | RTLD_NOLOAD) : nullptr;
    if (void *fn = unit ? dlsym(unit, "srs_jit_audit_drain_emu") : nullptr) {
        uint64_t counts[f29_audit::KIND_COUNT];
        char sites[f29_audit::KIND_COUNT][f29_audit::SITE_BYTES];
        reinterpret_cast<void (*)(unsigned long long *, char *)>(fn)(reinterpret_cast<unsigned long long *>(counts), &sites[0][0]);
        for (int kind = 0; kind < f29_audit::KIND_COUNT; ++kind)
            if (counts[kind]) f29_audit::table().add(kind, counts[kind], sites[kind]);
    }
    if (unit) dlclose(unit);                                 // the reference RTLD_NOLOAD took
#endif
    return true;
}

}  // namespace jit
}  // namespace srs
