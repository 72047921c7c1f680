// Issue cost on gfx950 of the 64-bit-rate vector instructions of k_table_build's
// item loop, next to v_fma_f32: v_mov_b64, v_lshl_add_u64,
// v_cvt_f64_f32, v_cvt_f32_f64, v_add_f64, v_mul_f64, v_fma_f64, v_floor_f64.
// Every lane runs 8 independent chains of one instruction (inline asm, so the
// stream is what is named); at most 4 or 7 waves per SIMD are resident, set
// by the blocks' LDS size (a block is 4 waves, one per SIMD), and the grid is
// 8 times that.  Output: SIMD cycles per wave64 instruction = the launch's
// time x shader clock x SIMDs / wave-instructions issued; the shader clock is
// s_memtime against s_memrealtime (100 MHz), and the waves actually resident
// per SIMD (the waves' summed clocks over the launch's) are printed beside
// it.  Build and run:
//   hipcc -O2 --offload-arch=gfx950 -o /tmp/valu64_microbench tools/probes/valu64_microbench.hip && /tmp/valu64_microbench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

constexpr int kIters = 2048, kRep = 4, kChains = 8;
struct Stamp { unsigned long long t0, t1, r0, r1; };

#define BODY(DECL, INIT, ASM, SINK)                                                       \
  extern __shared__ char lds[];                                                           \
  DECL;                                                                                   \
  for (int i = 0; i < kChains; ++i) { INIT; }                                             \
  __syncthreads();                                                                        \
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();                             \
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();                         \
  for (int it = 0; it < kIters; ++it) {                                                   \
    _Pragma("unroll") for (int r = 0; r < kRep; ++r) {                                    \
      _Pragma("unroll") for (int i = 0; i < kChains; ++i) { ASM; }                        \
    }                                                                                     \
  }                                                                                       \
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();                             \
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();                         \
  double s = 0;                                                                           \
  for (int i = 0; i < kChains; ++i) s += SINK;                                            \
  if (n < 0) lds[threadIdx.x] = (char)s; /* (keeps the dynamic LDS) */                    \
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;                                         \
  if ((threadIdx.x & 63) == 0) st[blockIdx.x * 4 + threadIdx.x / 64] = Stamp{t0, t1, r0, r1};

__global__ void k_fma_f32(double* out, Stamp* st, int n) {
  BODY(float x[kChains]; float a = 1.0001f; float b = 1e-4f, x[i] = threadIdx.x * 1e-3f + i,
       asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "v"(b)), (double)x[i])
}
__global__ void k_mov_b64(double* out, Stamp* st, int n) {
  BODY(double x[kChains]; double y[kChains], (x[i] = threadIdx.x + i, y[i] = i),
       asm volatile("v_mov_b64 %0, %1" : "=v"(r & 1 ? x[i] : y[i]) : "v"(r & 1 ? y[i] : x[i])),
       x[i] + y[i])
}
__global__ void k_lshl_add_u64(double* out, Stamp* st, int n) {
  BODY(unsigned long long x[kChains]; unsigned long long c = 0x9E3779B97F4A7C15ull,
       x[i] = threadIdx.x + i,
       asm volatile("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(x[i]) : "v"(c)), (double)x[i])
}
__global__ void k_cvt_f64_f32(double* out, Stamp* st, int n) {
  BODY(double x[kChains]; float f[kChains], (x[i] = 0.0, f[i] = threadIdx.x * 1e-3f + i),
       asm volatile("v_cvt_f64_f32 %0, %1" : "+v"(x[i]) : "v"(f[i])), x[i])
}
__global__ void k_cvt_f32_f64(double* out, Stamp* st, int n) {
  BODY(double x[kChains]; float f[kChains], (x[i] = threadIdx.x * 1e-3 + i, f[i] = 0.0f),
       asm volatile("v_cvt_f32_f64 %0, %1" : "+v"(f[i]) : "v"(x[i])), (double)f[i])
}
__global__ void k_add_f64(double* out, Stamp* st, int n) {
  BODY(double x[kChains]; double c = 1e-4, x[i] = threadIdx.x * 1e-3 + i,
       asm volatile("v_add_f64 %0, %0, %1" : "+v"(x[i]) : "v"(c)), x[i])
}
__global__ void k_mul_f64(double* out, Stamp* st, int n) {
  BODY(double x[kChains]; double c = 1.0000001, x[i] = threadIdx.x * 1e-3 + i + 1,
       asm volatile("v_mul_f64 %0, %0, %1" : "+v"(x[i]) : "v"(c)), x[i])
}
__global__ void k_fma_f64(double* out, Stamp* st, int n) {
  BODY(double x[kChains]; double a = 1.0000001; double b = 1e-4, x[i] = threadIdx.x * 1e-3 + i,
       asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "v"(b)), x[i])
}
__global__ void k_floor_f64(double* out, Stamp* st, int n) {
  BODY(double x[kChains], x[i] = threadIdx.x * 1e-3 + i + 0.5,
       asm volatile("v_floor_f64 %0, %0" : "+v"(x[i])), x[i])
}

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { \
  fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const int lds_cu = 160 * 1024;
  struct K { const char* name; void (*fn)(double*, Stamp*, int); } ks[] = {
    {"v_fma_f32", k_fma_f32}, {"v_mov_b64", k_mov_b64}, {"v_lshl_add_u64", k_lshl_add_u64},
    {"v_cvt_f64_f32", k_cvt_f64_f32}, {"v_cvt_f32_f64", k_cvt_f32_f64}, {"v_add_f64", k_add_f64},
    {"v_mul_f64", k_mul_f64}, {"v_fma_f64", k_fma_f64}, {"v_floor_f64", k_floor_f64}};
  const int kRounds = 8;
  const int max_blocks = cus * 7 * kRounds;
  double* out; Stamp* st;
  CHECK(hipMalloc(&out, (size_t)max_blocks * 256 * sizeof(double)));
  CHECK(hipMalloc(&st, (size_t)max_blocks * 4 * sizeof(Stamp)));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  Stamp* hs = (Stamp*)malloc((size_t)max_blocks * 4 * sizeof(Stamp));
  printf("%d CUs; %d instructions per wave; per column: SIMD shader clocks per wave64 "
         "instruction (waves resident per SIMD, shader clock in GHz)\n", cus,
         kIters * kRep * kChains);
  printf("%-16s %24s %24s\n", "instruction", "at most 4 waves/SIMD", "at most 7 waves/SIMD");
  for (auto& k : ks) {
    double cyc[2], res[2], ghz[2];
    for (int w = 0; w < 2; ++w) {
      const int wps = w == 0 ? 4 : 7;
      const int lds = (lds_cu / (wps + 1) + 1024) & ~1023;  // wps blocks of 4 waves fit a CU, not one more
      const int blocks = cus * wps * kRounds;
      CHECK(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k.fn, dim3(blocks), dim3(256), lds, 0, out, st, 0);
        CHECK(hipEventRecord(e1));
        CHECK(hipDeviceSynchronize());
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        CHECK(hipMemcpy(hs, st, (size_t)blocks * 4 * sizeof(Stamp), hipMemcpyDeviceToHost));
        double clk = 0, real = 0;
        for (int b = 0; b < blocks * 4; ++b) {
          clk += (double)(hs[b].t1 - hs[b].t0);
          real += (double)(hs[b].r1 - hs[b].r0);
        }
        ghz[w] = clk / real * 0.1;  // s_memrealtime ticks at 100 MHz
        const double launch_clk = ms * 1e-3 * ghz[w] * 1e9, simds = cus * 4.0;
        cyc[w] = launch_clk * simds / ((double)blocks * 4 * kIters * kRep * kChains);
        res[w] = clk / (launch_clk * simds);
      }
    }
    printf("%-16s %10.2f (%4.2f, %4.2f) %10.2f (%4.2f, %4.2f)\n", k.name, cyc[0], res[0], ghz[0],
           cyc[1], res[1], ghz[1]);
  }
  return 0;
}
