// sr_overlap.h -- the one overlap test of the checks on a call's buffers.  No engine types and no HIP: the host-only plan
// headers take it too (sr_forced_plan.h, which tests/forced_plan/plan_check.cpp includes on a machine without a device).
#pragma once
#include <cstddef>
#include <cstdint>

namespace sr {

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  A null pointer or an empty range shares none.
inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

}  // namespace sr
