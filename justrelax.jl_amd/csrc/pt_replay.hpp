// pt_replay.hpp -- which iterations of a PT loop somebody observes, and how many unobserved ones lie ahead: the window every driver that replays runs of
// unobserved iterations as captured graphs walks.  No HIP header: g++ alone compiles it (tests/host/pt_replay_harness.cpp).
#pragma once
#include <cstdint>

namespace pt_replay {

// Observed iterations (1-based): the multiples of nout (a residual check follows them) and `last`, the last one the loop can run -- iterMax + 1 for the
// Stokes loops (iter <= iterMax), iterMax for the heat loop.  The number of the next observed iteration when `iter` (< last) are done:
inline int64_t next_observed(int64_t iter, int64_t nout, int64_t last)
{
    const int64_t nxt = (iter / nout + 1) * nout;
    return nxt < last ? nxt : last;
}
// the unobserved iterations from here that may go into a replay; hold_back of them, just before the observed one, stay out of it (never positive for nout = 1)
inline int64_t unobserved_run(int64_t iter, int64_t nout, int64_t last, int64_t hold_back = 0) { return next_observed(iter, nout, last) - 1 - hold_back - iter; }
inline bool observes_next(int64_t iter, int64_t nout, int64_t last) { return next_observed(iter, nout, last) == iter + 1; }

}   // namespace pt_replay
