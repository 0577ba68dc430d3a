// float instantiations of the register-staged generic GEMM launchers; see gemm_kernels.h
#include "gemm_kernels.h"
CMX_GEMM_GENERIC_INST(float)
