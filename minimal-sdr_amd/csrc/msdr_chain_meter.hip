// msdr_chain_meter.hip -- the S-meter's reducer and its launcher (a translation unit of its own; the metered chain kernels live with their frames).
#include "msdr_chain_meter.hiph"
#include "msdr_block.h"

namespace msdr {

// one thread per channel: the nseg partials of the channel in segment order (for the double sums the order is part of the result)
template <typename T>
__global__ __launch_bounds__(256) void meter_reduce_kernel(const T *__restrict__ part, T *__restrict__ d_meter, int channels, int nseg)
{
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= channels) return;
    T s = part[ch * nseg];
    for (int k = 1; k < nseg; k++) s += part[ch * nseg + k];
    d_meter[ch] = s;
}

template <typename T>
static hipError_t meter_reduce(hipStream_t stream, const T *part, T *d_meter, int channels, int nseg)
{
    if (!part || !d_meter || channels <= 0 || nseg <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meter_reduce_kernel<T>, dim3(((unsigned)channels + 255u) / 256u), dim3(256), 0, stream, part, d_meter, channels, nseg);
    return hipGetLastError();
}

hipError_t launch_meter_reduce(hipStream_t stream, const unsigned long long *part, unsigned long long *d_meter, int channels, int nseg)
{
    return meter_reduce(stream, part, d_meter, channels, nseg);
}
hipError_t launch_meter_reduce(hipStream_t stream, const double *part, double *d_meter, int channels, int nseg)
{
    return meter_reduce(stream, part, d_meter, channels, nseg);
}

}  // namespace msdr
