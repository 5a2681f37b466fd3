// ulp_probe.hip -- the worst error, in ulps, of the device's exp, log and log1p as the smoothed value kernels call them
// (csrc/mhs_smooth.hpp: std::exp, std::log, std::log1p on double and on float, no fast-math flag), on fixed dense grids:
//   exp     on [-104, 0]   uniform
//   log     on [1, 2^24]   uniform, and geometric (the sums the kernels take the log of start at 1)
//   log1p   on [0, 1]      uniform
// 2^20 + 1 points each, both types.  Every result is compared with the host's expl / logl / log1pl on the same input
// (a float input is the rounded grid point); an ulp is the spacing of the type at the exact result, the subnormal
// spacing where the result is subnormal.  Prints one line per function and type -- the worst error over the grid and
// over the part of it whose exact result is normal -- and the constants c_exp and c_log that follow: the worst,
// rounded up to an integer, plus 1 (sampling does not meet the worst case).
// A stand-alone program:  hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ulp_probe.hip -o tools/ulp_probe
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#define HIP_OK(call)                                                                          \
    do {                                                                                      \
        const hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                               \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

enum Fn : int { FN_EXP, FN_LOG, FN_LOG1P };

template <class V>
__global__ __launch_bounds__(256) void k_eval(int fn, const V* __restrict__ x, V* __restrict__ y, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        y[i] = fn == FN_EXP ? std::exp(x[i]) : fn == FN_LOG ? std::log(x[i]) : std::log1p(x[i]);
}

constexpr int N = (1 << 20) + 1;

template <class V>
struct Type;
template <>
struct Type<double> {
    static constexpr int digits = DBL_MANT_DIG, min_exp = DBL_MIN_EXP;
    static constexpr const char* name = "f64";
};
template <>
struct Type<float> {
    static constexpr int digits = FLT_MANT_DIG, min_exp = FLT_MIN_EXP;
    static constexpr const char* name = "f32";
};

struct Worst {
    double all = 0, normal = 0;
    long double at = 0;
};

// the worst error of fn over x[0, N), in ulps of V at the exact result
template <class V>
int probe(int fn, const char* label, const std::vector<V>& x, Worst& w) {
    V *dx = nullptr, *dy = nullptr;
    std::vector<V> y(N);
    HIP_OK(hipMalloc((void**)&dx, sizeof(V) * N));
    HIP_OK(hipMalloc((void**)&dy, sizeof(V) * N));
    HIP_OK(hipMemcpy(dx, x.data(), sizeof(V) * N, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_eval<V>), dim3(1024), dim3(256), 0, 0, fn, dx, dy, N);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(y.data(), dy, sizeof(V) * N, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(dx));
    HIP_OK(hipFree(dy));
    Worst here;
    for (int i = 0; i < N; ++i) {
        const long double xi = x[i];
        const long double exact = fn == FN_EXP ? expl(xi) : fn == FN_LOG ? logl(xi) : log1pl(xi);
        if (exact == 0) {  // log(1), log1p(0): the result must be exactly 0
            if (y[i] != 0) here.all = here.normal = INFINITY, here.at = xi;
            continue;
        }
        int e = ilogbl(fabsl(exact));
        const bool normal = e >= Type<V>::min_exp - 1;
        if (!normal) e = Type<V>::min_exp - 1;
        const double err = (double)(fabsl((long double)y[i] - exact) / ldexpl(1.0L, e - (Type<V>::digits - 1)));
        if (err > here.all) here.all = err, here.at = xi;
        if (normal && err > here.normal) here.normal = err;
    }
    std::printf("%-15s %s  points %d  worst %.4f ulp (at x = %.17Lg)  worst over normal results %.4f ulp\n", label,
                Type<V>::name, N, here.all, here.at, here.normal);
    if (here.all > w.all) w.all = here.all;
    if (here.normal > w.normal) w.normal = here.normal;
    return 0;
}

template <class V>
std::vector<V> uniform(long double lo, long double hi) {
    std::vector<V> x(N);
    for (int i = 0; i < N; ++i) x[i] = (V)(lo + (hi - lo) * i / (N - 1));
    return x;
}
template <class V>
std::vector<V> geometric(long double lo, long double hi) {
    std::vector<V> x(N);
    for (int i = 0; i < N; ++i) x[i] = (V)(lo * powl(hi / lo, (long double)i / (N - 1)));
    x[0] = (V)lo, x[N - 1] = (V)hi;
    return x;
}

template <class V>
int probe_type() {
    Worst e, l;
    if (probe<V>(FN_EXP, "exp uniform", uniform<V>(-104, 0), e)) return 1;
    if (probe<V>(FN_LOG, "log uniform", uniform<V>(1, 16777216), l)) return 1;
    if (probe<V>(FN_LOG, "log geometric", geometric<V>(1, 16777216), l)) return 1;
    if (probe<V>(FN_LOG1P, "log1p uniform", uniform<V>(0, 1), l)) return 1;
    std::printf("%s: c_exp = ceil(%.4f) + 1 = %d   c_log = ceil(%.4f) + 1 = %d\n", Type<V>::name, e.all, (int)std::ceil(e.all) + 1,
                l.all, (int)std::ceil(l.all) + 1);
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, 0));
    std::printf("device: %s (%s)\n", prop.name, prop.gcnArchName);
    if (probe_type<double>()) return 1;
    if (probe_type<float>()) return 1;
    return 0;
}
