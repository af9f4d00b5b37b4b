// pe_hd.h -- how the host + device headers (fp381_s29.h, fp381_s30.h, the text they share and the point layers over them)
// declare a function, a static member and a constant table, so that the same text compiles under hipcc and under a plain
// host compiler.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PE_HD __host__ __device__ __forceinline__
#define PE_HD_MEMBER static __host__ __device__ __forceinline__
#else
#define PE_HD static inline
#define PE_HD_MEMBER static inline
#endif
#define PE_HD_CONST static constexpr  // constant-initialised: hipcc emits them for the device where device code reads them
