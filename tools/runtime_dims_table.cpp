// Prints runtime_dims' LDS and workspace sizes for every horizon the configuration check accepts and the four kinds of
// the runtime-sized kernels (plain, sensitivity, adjoint, adjoint_record), one line each: the table two builds must agree on when the LDS
// carve-up (csrc/vsmpc_rt_core.hpp) or runtime_dims (csrc/vsmpc_runtime.hip) is restated.  Host code only, no HIP call.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I <pkg>/csrc -c tools/runtime_dims_table.cpp -o dims_table.o
//   hipcc --offload-arch=gfx950 dims_table.o <pkg>/build/vsmpc_runtime.o -o dims_table
//   ./dims_table > new.txt      (the same in the other tree)      diff old.txt new.txt
#include <cstdio>

#include "vsmpc_launch.hpp"

int main() {
    using namespace vsmpc;
    std::printf("n ns hc kind lds_doubles ws_doubles lds_bytes tuned_lds_bytes\n");
    for (int n = 2; n <= MAX_STAGES; ++n)                  // config_valid (csrc/vsmpc_capi.hip): 2 <= ns <= hc <= n <= 40
        for (int hc = 2; hc <= n; ++hc)
            for (int ns = 2; ns <= hc; ++ns)
                for (int kind = 0; kind < 4; ++kind) {
                    const RtDims d = runtime_dims(n, ns, hc, kind == 1, kind >= 2, kind == 3);
                    const char* const names[4] = {"plain", "sensitivity", "adjoint", "adjoint_record"};
                    std::printf("%d %d %d %s %d %d %zu %zu\n", n, ns, hc, names[kind],
                                d.lds_doubles, d.ws_doubles, runtime_lds_bytes(d), runtime_tuned_lds_bytes(d));
                }
    return 0;
}
