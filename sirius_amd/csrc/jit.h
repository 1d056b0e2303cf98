// jit.h -- run-time compilation of straight-line row programs with hiprtc (see jit.hip).
#pragma once
#include <string>

#include "devrt.h"

namespace srs {
namespace jit {

struct Kernel {
    void *module = nullptr;     // hipModule_t
    void *function = nullptr;   // hipFunction_t
    double compile_seconds = 0;
};

// hiprtc present and not disabled (SRS_NO_JIT)
bool enabled();
// Compiles `source` for gfx950 (it may #include "field.cuh" and "rowprog_dev.cuh": the library carries their text) and
// loads `entry`.  false + log on failure; never throws.
bool compile(const std::string &source, const char *entry, Kernel &out, std::string &log);
// The hiprtc half alone (no device, nothing loaded): does `source` compile against the embedded headers?
bool compile_only(const std::string &source, size_t *code_bytes, std::string &log);
void release(Kernel &k);
// grid x 128 threads, `smem_bytes` of dynamic LDS, one struct argument passed by value
bool launch(const Kernel &k, unsigned blocks, unsigned threads, unsigned smem_bytes, const void *arg_struct, hipStream_t st);

// ---- units with several kernels (the ProtoGalaxy leaf unit, rowprog.hip pg_leaf_unit): one module, one Kernel per entry
#if !defined(SRS_EMU)
// compile() for such a unit: `out` owns the module and holds `entry`
bool compile_unit(const std::string &source, const char *entry, Kernel &out, std::string &log);
// Another entry of the module `owner` was compiled into: out.function, with out.module left empty -- the module belongs to `owner`,
// and release(out) only forgets the function.  false + log when the module has no such entry.
bool entry(const Kernel &owner, const char *name, Kernel &out, std::string &log);
// launch() on a two-dimensional grid (blocks_x, blocks_y)
bool launch_grid(const Kernel &k, unsigned blocks_x, unsigned blocks_y, unsigned threads, unsigned smem_bytes, const void *arg_struct, hipStream_t st);
#endif

}  // namespace jit
}  // namespace srs

#if defined(SRS_EMU)
#include "jit_emu_units.h"   // the logic emulator's inline definitions of the three (tests/emu; the single-kernel half: tests/emu/jit_emu.cpp)
#endif
