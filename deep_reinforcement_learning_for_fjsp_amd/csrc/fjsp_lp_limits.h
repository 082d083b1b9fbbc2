// The size rules of the device simplex, stated once for the host and the device: which tableau an instance can need, what
// it takes of the LDS of a CU (lp_device_kernel) or of the scratch pool (lp_global_kernel), and the two kernels' limits.
// Users: choose_lp_service (fjsp_env.hip), generate_pack_kernel and the generated create (fjsp_generate.hip),
// fjsp_lp_global_bytes and the two kernels' own refusals.  tests/lp_cases.py and tests/lp_global_cases.py restate them
// independently.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace fjsp {

constexpr uint32_t kLpLdsLimit = 156 * 1024;   // LDS bytes lp_device_kernel may take (of the 160 KB of a CU)
constexpr int kLpLdsColumns = 512;             // its widest tableau: the objective row is 8 registers of a lane
constexpr int kLpGlobalRows = 256;             // lp_global_kernel: four row groups of 64 in a lane
constexpr int kLpGlobalColumns = 1536;         // ... and 24 chunks of 64 columns in LDS

// The largest tableau an instance of K operation types, M machines, nx eligible pairs and R kinds can need: every
// operation type but a kind's last has a precedence row
__host__ __device__ inline int lp_max_rows(int K, int M, int R) { return K + M + K - R; }
__host__ __device__ inline int lp_max_columns(int K, int M, int nx, int R) { return nx + 1 + lp_max_rows(K, M, R) + 1; }

// The sizes that decide an instance's tableau.  lp_worst_case: those of the largest tableau a generator's parameters admit --
// rows, columns and bytes all grow with K, M, nx and with K - R, so most arise at R_max kinds of J_max operations each
// (rows R_max (2 J_max - 1) + M_max) with every (operation type, machine) pair eligible on M_max machines
struct LpTableau { int K, M, nx, R; };
inline LpTableau lp_worst_case(int R_max, int J_max, int M_max) { return LpTableau{R_max * J_max, M_max, R_max * J_max * M_max, R_max}; }

// LDS bytes of lp_device_kernel for that tableau:
// tableau | column values (x extraction) | (spare) | basis | ... | col_of, prec list | staged inputs: p, Q, n_now, kB (the tail)
// (32 bits hold it: a batch has at most 256 operation types on 32 machines, 38 MB)
__host__ __device__ inline uint32_t lp_device_lds_bytes(int K, int M, int nx, int R, int MP) {
    const size_t nr = (size_t)K + M + (K - R), nc = (size_t)nx + 1 + nr + 1;
    const size_t bytes = nr * nc * 8 + nc * 8 + 2 * nr * 8 + nr * 4 + (size_t)K * M * 2 + (size_t)K * 2 + nr * 2 + (size_t)K * MP * 2 + (size_t)K * 8 + 128;
    return (uint32_t)((bytes + 15) & ~(size_t)15);
}

// Bytes of a scratch slot of lp_global_kernel for a tableau of nr rows x nc columns
__host__ __device__ inline size_t lp_global_slot_bytes(int nr, int nc) { return ((size_t)nr * (size_t)nc * 8 + 255) & ~(size_t)255; }

}  // namespace fjsp
