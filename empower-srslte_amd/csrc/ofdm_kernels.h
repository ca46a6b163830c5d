// Internal launch interface of the OFDM receive FFT (ofdm_kernels.hip).
#ifndef SRSGPU_OFDM_KERNELS_H
#define SRSGPU_OFDM_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsgpu {
// nsf subframes: in + i*in_stride (15 N samples), out + i*out_stride (14 x nre; 12 x nre with
// ext_cp); tw: N twiddles
// e^{-2 pi i k / N}; radices: 4-bit radix per stage (first stage in the low nibble)
hipError_t launch_ofdm_rx(const float2 *in, size_t in_stride, float2 *out, size_t out_stride, int nsf,
                          int N, int nre, const float2 *tw, uint32_t radices, int nstages, float scale,
                          bool ext_cp, hipStream_t st);
// the same from a table: rows is a device array of nsf device-readable pointers, each to one
// subframe's 15 N samples in format fmt (0 complex float, 1 int16 I/Q, 2 int8 I/Q; 16-byte aligned);
// integer samples enter the FFT as (float)v * in_scale
hipError_t launch_ofdm_rx_rows(const void *const *rows, int fmt, float in_scale, float2 *out, size_t out_stride,
                               int nsf, int N, int nre, const float2 *tw, uint32_t radices, int nstages, float scale,
                               bool ext_cp, hipStream_t st);
// transmit: nsf grids (14 x nre at in + i*in_stride) -> 15 N time samples at out + i*out_stride
hipError_t launch_ofdm_tx(const float2 *in, size_t in_stride, float2 *out, size_t out_stride, int nsf,
                          int N, int nre, const float2 *tw, uint32_t radices, int nstages, float scale,
                          bool ext_cp, hipStream_t st);
} // namespace srsgpu
#endif
