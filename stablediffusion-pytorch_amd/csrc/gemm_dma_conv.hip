// The LDS-DMA GEMM kernels of implicit-im2col A (convolution forward / data gradients): see gemm_dma.h.
#include "gemm_dma.h"

template hipError_t sdmi_gemm_impl::launch_dma_mode<SDMI_A_CONV>(int, const Args&, const EpiArgs&, dim3, hipStream_t, int, int);
