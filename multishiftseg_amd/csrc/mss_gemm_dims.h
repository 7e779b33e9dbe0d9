// Status codes and tile extents that host-only code (fwd_route.h and its stand-alone check) shares with the kernels: plain C++, no HIP type.
#pragma once

#define MSS_OK 0
#define MSS_ERR_BAD_ARG 1001     // a precondition of the C-ABI entry point was violated
#define MSS_ERR_UNSUPPORTED 1002 // shape outside what the kernels are built for

constexpr int MSS_GEMM_BM = 128;   // rows of a tile of the persistent GEMM kernels (gemm.hip, gemm_bf16x3.hip)
constexpr int MSS_GEMM_BK = 16;    // their K-step
constexpr int MSS_STEM7_K = 64;    // output channels of the 7x7 stem kernel (stem7.hip)
