// The LDS-DMA GEMM kernels of row-major A (linear forward / data gradients): see gemm_dma.h.
#include "gemm_dma.h"

template hipError_t sdmi_gemm_impl::launch_dma_mode<SDMI_A_ROWMAJOR>(int, const Args&, const EpiArgs&, dim3, hipStream_t, int,
                                                                int);
