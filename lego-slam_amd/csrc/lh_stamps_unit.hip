// lh_stamps_unit.hip — the diagnostic library's solver kernels as one translation unit, compiled with -DLH_STAMPS.
// lh_stamps (lh_dev.h) is one __device__ array that kernels of several files add into and lh_read_stamps reads;
// without relocatable device code it cannot span code objects, so the stamped kernels share this one.
#ifndef LH_STAMPS
#error "lh_stamps_unit.hip is the -DLH_STAMPS build of the solver's kernel files"
#endif
#define LH_STAMPS_UNIT   // lh_dev.h refuses LH_STAMPS anywhere else
#include "lh_lin.hip"
#include "lh_kernels.hip"
#include "lh_frames.hip"
#include "lh_aux.hip"
