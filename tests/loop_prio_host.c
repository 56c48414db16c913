/* loop_prio_host.c — prints llpf_loop_prio (csrc/shared/llpf_loop_prio.h) for every map and rounds_left = 0 .. 9, one line per map.
 * Build: cc -O1 -Wall -I <csrc>/shared loop_prio_host.c -o loop_prio_host   (tests/test_loop_priority_map.py) */
#include <stdio.h>
#include "llpf_loop_prio.h"

int main(void) {
    for (int map = 0; map <= 2; ++map) {
        printf("map %d:", map);
        for (int r = 0; r <= 9; ++r) printf(" %d", llpf_loop_prio(map, r));
        printf("\n");
    }
    return 0;
}
