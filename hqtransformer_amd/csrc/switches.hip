// The one place of csrc/ that reads the environment: the table of switches.h behind switch_value().  Plain C++ (no HIP header).
#include "switches.h"

#include <atomic>
#include <cstdint>
#include <cstdlib>

namespace {

struct SwitchRow { const char* var; SwitchParse parse; int dflt; SwitchRead read; };

const SwitchRow SWITCH_ROWS[SW_COUNT] = {
#define X(id, var, parse, dflt, read, effect, who) {var, parse, dflt, read},
    SWITCH_TABLE(X)
#undef X
};

int switch_parse(const SwitchRow& r) {
    const char* e = getenv(r.var);
    switch (r.parse) {
    case SWP_PRESENT: return e != nullptr;
    case SWP_ZERO_OFF: return !(e && atoi(e) == 0);
    case SWP_INT: return e ? atoi(e) : r.dflt;
    case SWP_INT_MIN1: return e ? (atoi(e) > 1 ? atoi(e) : 1) : r.dflt;
    case SWP_INT_8_OR_16: { const int v = e ? atoi(e) : 0; return v == 8 || v == 16 ? v : 0; }
    }
    return r.dflt;
}

// SWR_ONCE: 0 = not read yet, else bit 32 | the value.  The first thread to store decides; a thread that loses the race takes the winner's value.
std::atomic<int64_t> switch_first_read[SW_COUNT];

}  // namespace

int switch_value(Switch s) {
    const SwitchRow& r = SWITCH_ROWS[s];
    if (r.read == SWR_LIVE) return switch_parse(r);
    int64_t seen = switch_first_read[s].load(std::memory_order_acquire);
    if (!seen) {
        const int64_t mine = (int64_t(1) << 32) | uint32_t(switch_parse(r));
        if (switch_first_read[s].compare_exchange_strong(seen, mine, std::memory_order_acq_rel)) seen = mine;
    }
    return int(uint32_t(seen));
}
