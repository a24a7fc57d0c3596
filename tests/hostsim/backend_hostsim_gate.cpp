// tests/hostsim/backend_hostsim_gate.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The hostsim backend's part for chained decodes of wide rows (linked into
// tests/hostsim/libsiamese_hostsim.so beside backend_hostsim.cpp, never into
// the product library):
//   * be_launch_ldpc_gated: k_ldpc with the per-item gate array (ops.h
//     LdpcItem); an item whose outcome word is zero is not run at all.
//   * be_launch_ge with a test hook.  backend_hostsim.cpp is compiled with
//     its be_launch_ge named be_launch_ge_plain (siamese_amd/Makefile); the
//     one here runs it and then, with SGPU_TEST_GE_FORCE_SINGULAR=1, makes
//     every chained job report a singular matrix (outcome word 0, stopped at
//     pivot 0).  What a successful job wrote for its solve stays, as that
//     solve is gated on the outcome and does not run.
#include "../../siamese_amd/csrc/backend.h"

#include <cstdlib>

namespace sgpu {

void be_launch_ge_plain(const GeDesc* descs, const uint8_t* in, uint32_t count, uint32_t* results, SolveRow* rows,
                        uint8_t* coef, uint32_t maxRows, uint32_t maxCols, const BeCopy* head, bool side,
                        const SolveRow* rowsIn);

void be_launch_ge(const GeDesc* descs, const uint8_t* in, uint32_t count, uint32_t* results, SolveRow* rows,
                  uint8_t* coef, uint32_t maxRows, uint32_t maxCols, const BeCopy* head, bool side,
                  const SolveRow* rowsIn)
{
    be_launch_ge_plain(descs, in, count, results, rows, coef, maxRows, maxCols, head, side, rowsIn);
    // (read per launch, so one test process can switch it)
    const char* force = std::getenv("SGPU_TEST_GE_FORCE_SINGULAR");
    if (!force || std::atol(force) == 0)
        return;
    for (uint32_t k = 0; k < count; ++k)
        if (descs[k].flags & kGeChained) {
            uint32_t* out = results + descs[k].result;
            out[0] = 0;   // the first pivot without a non-zero
            out[3] = 0;   // the outcome the gates read
        }
}

void be_launch_ldpc_gated(const LdpcItem* items, uint32_t count, uint64_t* acct, const uint32_t* gates,
                          const uint32_t* results)
{
    for (uint32_t k = 0; k < count; ++k) {
        // (a gated item of a chained elimination that failed)
        if (gates[k] != 0 && results[gates[k] - 1] == 0)
            continue;
        be_launch_ldpc(items + k, 1, acct);
    }
}

} // namespace sgpu
