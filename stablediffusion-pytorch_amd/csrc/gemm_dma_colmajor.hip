// The LDS-DMA GEMM kernels of col-major A (weight gradients, with their reduction columns): see gemm_dma.h.
#include "gemm_dma.h"

template hipError_t sdmi_gemm_impl::launch_dma_mode<SDMI_A_COLMAJOR>(int, const Args&, const EpiArgs&, dim3, hipStream_t, int,
                                                                int);
