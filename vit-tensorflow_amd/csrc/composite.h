// Host toolkit of the composite models (mim.hip, distill.hip, cross_vit.hip, cct.hip): a C-ABI handle that owns a public parameter / gradient
// arena in its own table order and drives one or more ViT engines.  Everything here is host code; kernels stay in their .hip files.
// A new composite starts from this header.
#pragma once
#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "engine.h"

int capi_fail(int code, const std::string& msg);   // capi.hip (thread-local last-error text)

// inside a function with a `std::string& err` in scope
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) {                                                                         \
      err = std::string(#x) + ": " + hipGetErrorString(e_);                                         \
      return VITX_ERR_HIP;                                                                          \
    }                                                                                               \
  } while (0)

// bodies of extern "C" functions: no exception crosses the boundary, HIP errors become the last-error text
#define CAPI_TRY try {
#define CAPI_CATCH                                                                    \
  }                                                                                   \
  catch (const std::exception& ex) { return capi_fail(VITX_ERR_INVALID, ex.what()); } \
  catch (...) { return capi_fail(VITX_ERR_INVALID, "unknown C++ exception"); }
#define CAPI_HIP(x)                                                                                        \
  do {                                                                                                     \
    hipError_t e_ = (x);                                                                                   \
    if (e_ != hipSuccess) return capi_fail(VITX_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));  \
  } while (0)

// Appends to a parameter table: `offset` counts the packed host blob, `aoff` the device arena (every tensor starts on a multiple of 4 elements).
struct TableBuilder {
  std::vector<ParamDesc>& t;
  int64_t n = 0, n_arena = 0;
  int64_t add(const std::string& name, std::vector<int64_t> shape) {   // -> arena offset
    ParamDesc p;
    p.name = name; p.shape = shape; p.count = 1;
    for (int64_t s : shape) p.count *= s;
    p.offset = n; p.aoff = n_arena;
    n += p.count;
    n_arena += round_up(p.count, 4);
    t.push_back(p);
    return p.aoff;
  }
};

// Device buffers of one handle, zeroed on `stream` when made.  free_all() only frees: the owner synchronises first.
struct DevicePool {
  std::vector<void*> ptrs;
  template <class T>
  int alloc(T** p, size_t bytes, hipStream_t stream, std::string& err) {
    bytes = (size_t)round_up((int64_t)std::max<size_t>(bytes, 16), 256);
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, bytes));
    HIPCHK(hipMemsetAsync(q, 0, bytes, stream));
    ptrs.push_back(q);
    *p = (T*)q;
    return VITX_OK;
  }
  void free_all() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};
// pool.alloc inside a create function (`err` in scope); ON_FAIL is what that function returns for the failure code rc_
#define POOL_ALLOC(pool, ptr, bytes, stream, ON_FAIL)                         \
  do {                                                                        \
    int rc_ = (pool).alloc(&(ptr), (size_t)(bytes), stream, err);             \
    if (rc_ != VITX_OK) return ON_FAIL;                                       \
  } while (0)

inline bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if (p && ((uintptr_t)p & 15)) return false;
  return true;
}
inline unsigned grid256(int64_t n) { return (unsigned)std::max<int64_t>(1, ceil_div(n, 256)); }

// Keras Dense on fp32 rows and its two VJPs, on the generic GEMM path (x3: the split-operand bf16 MFMA kernel where it applies)
// Y[M, N] = X[M, K] W[K, N] (+ bias)
inline void dense_fwd(const float* X, int64_t ldx, const float* W, const float* bias, float* Y, int M, int N, int K, hipStream_t s, int x3 = 0) {
  GenericGemmArgs g;
  g.A = X; g.B = W; g.M = M; g.N = N; g.K = K; g.sam = ldx; g.sak = 1; g.sbk = N; g.sbn = 1; g.x3 = x3;
  EpiParams ep;
  ep.out = Y; ep.ldo = N; ep.M = M; ep.N = N; ep.bias = bias; ep.vec_ok = (N % 4 == 0) && aligned16({Y, bias});
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
}
// dX[M, K] = dY[M, N] W[K, N]^T
inline void dense_dx(const float* dY, const float* W, float* dX, int M, int N, int K, hipStream_t s, int x3 = 0) {
  GenericGemmArgs g;
  g.A = dY; g.B = W; g.M = M; g.N = K; g.K = N; g.sam = N; g.sak = 1; g.sbk = 1; g.sbn = N; g.x3 = x3;
  EpiParams ep;
  ep.out = dX; ep.ldo = K; ep.M = M; ep.N = K; ep.vec_ok = (K % 4 == 0) && aligned16({dX});
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
}
// dW[K, N] = X[M, K]^T dY[M, N]
inline void dense_dw(const float* X, int64_t ldx, const float* dY, float* dW, int M, int N, int K, hipStream_t s, int x3 = 0) {
  GenericGemmArgs g;
  g.A = X; g.B = dY; g.M = K; g.N = N; g.K = M; g.sam = 1; g.sak = ldx; g.sbk = N; g.sbn = 1; g.x3 = x3;
  EpiParams ep;
  ep.out = dW; ep.ldo = N; ep.M = K; ep.N = N; ep.vec_ok = (N % 4 == 0) && aligned16({dW});
  launch_gemm_generic(g, ep, EPI_STORE_F32, 0, 0, 0, s);
}

// the body of every *_param_table_entry export
inline int write_table_entry(const std::vector<ParamDesc>& table, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                             int64_t* offset_elems) {
  if (index < 0 || index >= (int64_t)table.size()) return capi_fail(VITX_ERR_INVALID, "parameter index out of range");
  const ParamDesc& p = table[(size_t)index];
  if (name && name_cap > 0) { std::strncpy(name, p.name.c_str(), (size_t)name_cap - 1); name[name_cap - 1] = 0; }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = i < (int)p.shape.size() ? p.shape[(size_t)i] : 1;
  if (rank) *rank = (int32_t)p.shape.size();
  if (offset_elems) *offset_elems = p.offset;
  return VITX_OK;
}

// packed host blob <-> aligned device arena, tensor by tensor; `what` is the refusal of a blob of the wrong size
inline int copy_param_blob(const std::vector<ParamDesc>& table, int64_t n_params, float* arena, float* host, int64_t n, bool to_device,
                           hipStream_t stream, const char* what) {
  if (n != n_params) return capi_fail(VITX_ERR_INVALID, what);
  for (auto& p : table) {
    if (to_device) CAPI_HIP(hipMemcpyAsync(arena + p.aoff, host + p.offset, (size_t)p.count * 4, hipMemcpyHostToDevice, stream));
    else CAPI_HIP(hipMemcpyAsync(host + p.offset, arena + p.aoff, (size_t)p.count * 4, hipMemcpyDeviceToHost, stream));
  }
  CAPI_HIP(hipStreamSynchronize(stream));
  return VITX_OK;
}

// The arena exports of a composite that maps its arena onto its engines' (inside extern "C"): PFX##_handle has table, n_params, n_arena, params,
// grads and stream, and push_params(handle, err) copies the arena to the engines.  WHAT: copy_param_blob's refusal.
#define COMPOSITE_ARENA_EXPORTS(PFX, WHAT)                                                                         \
  int32_t PFX##_set_params(PFX##_handle m, const float* host_blob, int64_t n) {                                    \
    CAPI_TRY                                                                                                       \
    if (!m || !host_blob) return capi_fail(VITX_ERR_INVALID, "null argument");                                     \
    int rc = copy_param_blob(m->table, m->n_params, m->params, const_cast<float*>(host_blob), n, true, m->stream, WHAT); \
    if (rc != VITX_OK) return rc;                                                                                  \
    std::string err;                                                                                               \
    if ((rc = push_params(m, err)) != VITX_OK) return capi_fail(rc, err);                                          \
    CAPI_HIP(hipStreamSynchronize(m->stream));                                                                     \
    return VITX_OK;                                                                                                \
    CAPI_CATCH                                                                                                     \
  }                                                                                                                \
  int32_t PFX##_get_params(PFX##_handle m, float* host_blob, int64_t n) {                                          \
    CAPI_TRY                                                                                                       \
    if (!m || !host_blob) return capi_fail(VITX_ERR_INVALID, "null argument");                                     \
    return copy_param_blob(m->table, m->n_params, m->params, host_blob, n, false, m->stream, WHAT);                \
    CAPI_CATCH                                                                                                     \
  }                                                                                                                \
  int32_t PFX##_get_grads(PFX##_handle m, float* host_blob, int64_t n) {                                           \
    CAPI_TRY                                                                                                       \
    if (!m || !host_blob) return capi_fail(VITX_ERR_INVALID, "null argument");                                     \
    return copy_param_blob(m->table, m->n_params, m->grads, host_blob, n, false, m->stream, WHAT);                 \
    CAPI_CATCH                                                                                                     \
  }                                                                                                                \
  int32_t PFX##_params_dev(PFX##_handle m, float** dev_ptr, int64_t* n_elems) {                                    \
    if (!m || !dev_ptr) return capi_fail(VITX_ERR_INVALID, "null argument");                                       \
    *dev_ptr = m->params;                                                                                          \
    if (n_elems) *n_elems = m->n_arena;                                                                            \
    return VITX_OK;                                                                                                \
  }                                                                                                                \
  int32_t PFX##_grads_dev(PFX##_handle m, float** dev_ptr, int64_t* n_elems) {                                     \
    if (!m || !dev_ptr) return capi_fail(VITX_ERR_INVALID, "null argument");                                       \
    *dev_ptr = m->grads;                                                                                           \
    if (n_elems) *n_elems = m->n_arena;                                                                            \
    return VITX_OK;                                                                                                \
  }                                                                                                                \
  int32_t PFX##_params_changed(PFX##_handle m) {                                                                   \
    CAPI_TRY                                                                                                       \
    if (!m) return capi_fail(VITX_ERR_INVALID, "null handle");                                                     \
    std::string err;                                                                                               \
    int rc = push_params(m, err);                                                                                  \
    if (rc != VITX_OK) return capi_fail(rc, err);                                                                  \
    return VITX_OK;                                                                                                \
    CAPI_CATCH                                                                                                     \
  }
