// tune.cpp -- the tuning table (every ACG_* measurement / layout switch), its look-ups for the launchers and the host units,
// and what says which build this is.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>

#include "acarsdec_amd.h"
#include "acarsdec_amd_lab.h"


extern char** environ;

namespace {


// ---- tuning overrides --------------------------------------------------------------------------------------------
// Every measurement / layout switch of the library (ACG_FIR_VARIANT, ACG_MSK_LPC, ACG_PIPE_BLOCKS, ...) lives in ONE table.
// A production process has an EMPTY table: a look-up is then one relaxed atomic load and returns the default -- no mutex,
// no string, no allocation on any launch path.  The table gets entries in two ways only:
//   * acg_tune(name, value) (bench.py --ab, the tests' `tune` fixture, the probes);
//   * the environment, read ONCE at the first look-up of the process and reported on stderr -- in the product library only
//     when ACG_ALLOW_TUNING=1 is set as well (a stray ACG_* variable of a host process is then named on stderr and ignored);
//     the lab build (libacarsdec_amd_lab.so, -DACG_LAB: tests and probes) always takes it.
// The measurement-only kernels and debug shapes (FIR variants other than 5 / 3, ACG_FIR_DEBUG_*, the two-wave demodulator)
// are not compiled into the product library at all.
std::mutex g_tune_mx;
std::map<std::string, std::string> g_tune;
std::atomic<int> g_tune_state{0};            // 0 = environment not looked at yet, 1 = table empty, 2 = table has entries

void tune_init_locked()
{
    if (g_tune_state.load(std::memory_order_relaxed) != 0) return;
    std::string seen;
    bool allow = false;
#ifdef ACG_LAB
    allow = true;
#endif
    for (char** e = environ; e && *e; ++e)
        if (std::strcmp(*e, "ACG_ALLOW_TUNING=1") == 0) allow = true;
    for (char** e = environ; e && *e; ++e) {
        const char* kv = *e;
        if (std::strncmp(kv, "ACG_", 4) != 0 || std::strncmp(kv, "ACG_BENCH_", 10) == 0 || std::strncmp(kv, "ACG_ALLOW_TUNING", 16) == 0) continue;
        const char* eq = std::strchr(kv, '=');
        if (!eq) continue;
        if (allow) g_tune[std::string(kv, (size_t)(eq - kv))] = std::string(eq + 1);
        seen += std::string(" ") + kv;
    }
    if (!seen.empty())
        std::fprintf(stderr, allow ? "acarsdec_amd: tuning overrides taken from the environment (measurement switches, not product "
                                     "configuration):%s\n"
                                   : "acarsdec_amd: ACG_* variables in the environment IGNORED (they are measurement switches; set "
                                     "ACG_ALLOW_TUNING=1 to apply them):%s\n", seen.c_str());
    g_tune_state.store(g_tune.empty() ? 1 : 2, std::memory_order_release);
}

}  // namespace

// look-up used by the launchers (fir.hip, msk.hip) and this file: the override's integer value, or dflt
extern "C" int acg_tune_get(const char* name, int dflt)
{
    if (g_tune_state.load(std::memory_order_acquire) == 1) return dflt;          // the production case: nothing to look up
    std::lock_guard<std::mutex> lk(g_tune_mx);
    tune_init_locked();
    if (g_tune.empty()) return dflt;
    auto it = g_tune.find(name);
    return it == g_tune.end() ? dflt : std::atoi(it->second.c_str());
}
extern "C" int acg_tune_has(const char* name)
{
    if (g_tune_state.load(std::memory_order_acquire) == 1) return 0;
    std::lock_guard<std::mutex> lk(g_tune_mx);
    tune_init_locked();
    return g_tune.count(name) ? 1 : 0;
}
extern "C" int acg_tune(const char* name, const char* value)
{
    if (!name || std::strncmp(name, "ACG_", 4) != 0) return ACG_EINVAL;
    std::lock_guard<std::mutex> lk(g_tune_mx);
    tune_init_locked();
    if (value) g_tune[name] = value;
    else g_tune.erase(name);
    g_tune_state.store(g_tune.empty() ? 1 : 2, std::memory_order_release);
    return ACG_OK;
}
// 1 in the lab build (libacarsdec_amd_lab.so: every kernel variant and debug shape), 0 in the product library
extern "C" int acg_is_lab_build(void)
{
#ifdef ACG_LAB
    return 1;
#else
    return 0;
#endif
}
