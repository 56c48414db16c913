/* llpf_loop_prio.h — wave priority of a round of the fused timestep's output loop, from the rounds the wave still has to do.
 *
 * The waves of a SIMD are served by priority, then by age.  At one priority the wave of the block dispatched first runs all of its rounds
 * first and the youngest block's wave runs its rounds last, alone on the SIMD (kernels/resprop.hpp: wave priority by phase).  A wave that
 * sets its priority from the rounds it has left (the round it is about to run included) wins arbitration against every wave that is
 * further along; waves at equal progress fall back to age.  The last round of every wave runs at priority 0.
 *
 *   map 1 (A): min(2, rounds_left - 1)   priority 3 stays reserved for head, counts and tail
 *   map 2 (B): min(3, rounds_left - 1)
 *   map 0    : no priority by progress (0)
 *
 * A value for s_setprio, which takes an immediate: the kernel branches on it.  Shared with the host so that a CPU test can pin the map.
 */
#ifndef LLPF_LOOP_PRIO_H
#define LLPF_LOOP_PRIO_H

#ifndef LLPF_HD
#include "llpf_detmath.h"
#endif

LLPF_HD int llpf_loop_prio(int map, int rounds_left) {
    const int top = map == 1 ? 2 : (map == 2 ? 3 : 0);
    const int p = rounds_left - 1;
    return p < 0 ? 0 : (p < top ? p : top);
}

#endif
