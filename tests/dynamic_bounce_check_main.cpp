// Host-only driver of what vct_set_dynamic_bounce added to csrc/vct_dynamic_check.h -- the switch's argument check, the
// bytes of the bounce's brick -> resolved-slot table and the slots its list kernel is sized for -- for a run under
// -fsanitize=address,undefined (tests/test_dynamic_bounce_host.py).  No GPU call.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_dynamic_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    // the switch: 0 or 1
    EXPECT(!vct_dynamic_check_bounce(0) && !vct_dynamic_check_bounce(1));
    EXPECT(vct_dynamic_check_bounce(-1) && vct_dynamic_check_bounce(2) && vct_dynamic_check_bounce(INT32_MAX) && vct_dynamic_check_bounce(INT32_MIN));

    // the table: one word per brick of the grid, nothing for no grid
    EXPECT(vct_dynamic_bounce_map_bytes(8) == 4u && vct_dynamic_bounce_map_bytes(16) == 32u && vct_dynamic_bounce_map_bytes(64) == 2048u);
    EXPECT(vct_dynamic_bounce_map_bytes(512) == 262144u * 4u && vct_dynamic_bounce_map_bytes(1024) == 2097152u * 4u);
    EXPECT(vct_dynamic_bounce_map_bytes(4) == 0u && vct_dynamic_bounce_map_bytes(0) == 0u && vct_dynamic_bounce_map_bytes(-64) == 0u);
    for (int32_t V = 8; V <= 1024; V *= 2) {
        // the table of exactly that size takes the entry of the grid's last brick, filled as the host fills it
        std::vector<unsigned char> table(vct_dynamic_bounce_map_bytes(V));
        memset(table.data(), 0xff, table.size());
        const uint32_t last = vct_dynamic_grid_bricks(V) - 1u, slot = 7u;
        memcpy(table.data() + (size_t)last * sizeof(uint32_t), &slot, sizeof(slot));
        uint32_t first = 0u;
        memcpy(&first, table.data(), sizeof(first));
        EXPECT(table.size() == (size_t)vct_dynamic_grid_bricks(V) * 4u && (last == 0u || first == 0xffffffffu));
    }

    // the list kernel's slots: the static ones and the layer's behind them
    EXPECT(vct_dynamic_bounce_list_slots(0u, 0u) == 0u && vct_dynamic_bounce_list_slots(283u, 64u) == 347u);
    EXPECT(vct_dynamic_bounce_list_slots(2097152u, 2097152u) == 4194304u);      // the largest grid, every brick twice
    EXPECT(vct_dynamic_bounce_list_slots(0xffffffffu, 1u) == 0xffffffffu && vct_dynamic_bounce_list_slots(0xffffffffu, 0xffffffffu) == 0xffffffffu);
    EXPECT(vct_dynamic_bounce_list_slots(0xfffffffeu, 1u) == 0xffffffffu && vct_dynamic_bounce_list_slots(0u, 0xffffffffu) == 0xffffffffu);

    if (failures) { printf("dynamic_bounce_check: %d failures\n", failures); return 1; }
    printf("dynamic_bounce_check ok\n");
    return 0;
}
