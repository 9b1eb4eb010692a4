// Host toolkit of the eight composite models (mim.hip, distill.hip, cross_vit.hip, cct.hip, nest.hip, twins.hip, cvt.hip, crossformer.hip): a C-ABI handle that
// owns a public parameter / gradient arena in its own table order and drives one or more ViT engines.  Here: error plumbing, TableBuilder,
// DevicePool, the Dense products, the table / blob exports, the arena maps (ArenaMap, add_arena_map, copy_maps), the profiler scope and the
// begin / end bodies over a handle's engines, and the bodies of the create / host forward / host backward / read exports.  Everything here is
// host code; kernels stay in their .hip files.  A new composite starts from this header.
#pragma once
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <map>

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

// ---------------------------------------------------------------------------------------------- arena maps
// A tensor of the composite's arena (or a column block of the engine's) and where it lives in an engine's: `rows` pieces of `width` floats,
// `epitch` apart in the engine; rows == 1 is one contiguous run.
struct ArenaMap { int64_t c, e, rows, width, epitch; };

inline const ParamDesc* find_desc(const std::vector<ParamDesc>& t, const std::string& n) {
  for (const auto& p : t) if (p.name == n) return &p;
  return nullptr;
}

// Appends the map of the composite's tensor `cname` onto the engine's `ename`.  width < 0: the whole tensor, one run of its span (the count
// rounded up to the 4-element tensor alignment of both arenas; the padding is in no table), merged into the run before it when the two are
// adjacent in both arenas.  Otherwise the composite tensor is the column block [col0, col0 + width) of the engine's (to_q | to_kv -> to_qkv).
inline int add_arena_map(std::vector<ArenaMap>& maps, const std::vector<ParamDesc>& ctable, const std::string& cname, const std::vector<ParamDesc>& etable,
                         const std::string& ename, std::string& err, int64_t col0 = 0, int64_t width = -1) {
  const ParamDesc *cp = find_desc(ctable, cname), *ep = find_desc(etable, ename);
  bool ok = cp && ep && (width < 0 ? cp->count == ep->count : width > 0 && cp->count % width == 0 && ep->count % (cp->count / width) == 0);
  const int64_t rows = ok && width > 0 ? cp->count / width : 1, epitch = ok && width > 0 ? ep->count / rows : 0;
  if (ok && width > 0) ok = col0 >= 0 && col0 + width <= epitch;
  if (!ok) { err = "internal: parameter map " + cname + " -> " + ename; return VITX_ERR_INVALID; }
  if (width > 0) { maps.push_back({cp->aoff, ep->aoff + col0, rows, width, epitch}); return VITX_OK; }
  const int64_t span = round_up(cp->count, 4);
  if (!maps.empty() && maps.back().rows == 1 && maps.back().c + maps.back().width == cp->aoff && maps.back().e + maps.back().width == ep->aoff) {
    maps.back().width += span; maps.back().epitch += span;
  } else maps.push_back({cp->aoff, ep->aoff, 1, span, span});
  return VITX_OK;
}

// composite arena -> engine arena (to_engine) or back, on `stream`
inline int copy_maps(float* arena, float* engine_arena, const std::vector<ArenaMap>& maps, bool to_engine, hipStream_t stream, std::string& err) {
  for (const ArenaMap& t : maps) {
    float *cp = arena + t.c, *ep = engine_arena + t.e;
    if (t.rows == 1) HIPCHK(hipMemcpyAsync(to_engine ? ep : cp, to_engine ? cp : ep, (size_t)t.width * 4, hipMemcpyDeviceToDevice, stream));
    else if (to_engine) HIPCHK(hipMemcpy2DAsync(ep, (size_t)t.epitch * 4, cp, (size_t)t.width * 4, (size_t)t.width * 4, (size_t)t.rows, hipMemcpyDeviceToDevice, stream));
    else HIPCHK(hipMemcpy2DAsync(cp, (size_t)t.width * 4, ep, (size_t)t.epitch * 4, (size_t)t.width * 4, (size_t)t.rows, hipMemcpyDeviceToDevice, stream));
  }
  return VITX_OK;
}

// ---------------------------------------------------------------------------------------------- profiler
// a launch (or a group of launches) of a composite booked under a kernel class of an engine's profiler (vitx_*_profile_*); a null engine (a
// handle none of whose stages has blocks) profiles nothing
struct CompositeProf {
  vitx_engine* e;
  ProfEvent pe{};
  bool on;
  CompositeProf(vitx_engine* e_, const char* name) : e(e_), on(e_ && e_->profiling) {
    if (!on) return;
    pe.cls = prof_class(e, name);
    pe.cls2 = -1; pe.flops = 0; pe.bytes = 0;
    (void)hipEventCreate(&pe.e0);
    (void)hipEventCreate(&pe.e1);
    (void)hipEventRecord(pe.e0, e->stream);
  }
  ~CompositeProf() {
    if (!on) return;
    (void)hipEventRecord(pe.e1, e->stream);
    e->prof_events.push_back(pe);
  }
};

// the bodies of vitx_*_profile_begin / _end over the engines of a handle
inline int composite_profile_begin(const std::vector<vitx_engine*>& engs) {
  CAPI_TRY
  for (size_t i = 0; i < engs.size(); ++i) {
    const int rc = vitx_profile_begin(engs[i]);
    if (rc == VITX_OK) continue;
    for (size_t j = 0; j < i; ++j) (void)vitx_profile_end(engs[j], nullptr, 0, nullptr);   // leave no engine profiling behind a failure
    return rc;
  }
  return VITX_OK;
  CAPI_CATCH
}
// the engines each keep their own classes: the same class of several engines is summed
inline int composite_profile_end(const std::vector<vitx_engine*>& engs, vitx_kernel_stat* out, int32_t cap, int32_t* n_out) {
  CAPI_TRY
  std::vector<vitx_kernel_stat> all, one(256);
  int first_err = VITX_OK;
  std::map<std::string, size_t> at;
  for (vitx_engine* eng : engs) {
    int32_t k = 0;
    const int rc = vitx_profile_end(eng, one.data(), (int32_t)one.size(), &k);
    if (rc != VITX_OK) { if (first_err == VITX_OK) first_err = rc; continue; }   // (the other engines still stop profiling and release their events)
    for (int32_t j = 0; j < std::min<int32_t>(k, (int32_t)one.size()); ++j) {
      const auto it = at.find(one[(size_t)j].name);
      if (it == at.end()) { at[one[(size_t)j].name] = all.size(); all.push_back(one[(size_t)j]); continue; }
      vitx_kernel_stat& t = all[it->second];
      t.launches += one[(size_t)j].launches; t.total_ms += one[(size_t)j].total_ms; t.flops += one[(size_t)j].flops; t.bytes += one[(size_t)j].bytes;
    }
  }
  if (first_err != VITX_OK) return first_err;
  for (size_t j = 0; j < all.size() && out && (int32_t)j < cap; ++j) out[j] = all[j];
  if (n_out) *n_out = (int32_t)all.size();
  return VITX_OK;
  CAPI_CATCH
}

// ---------------------------------------------------------------------------------------------- C-ABI bodies
// of the composites created from a config: M has cfg.max_batch, stream, img, dimg, logits, dlogits, nc, b and have_fwd; the extern "C" function
// checks its pointers and passes the model's own function.
// TABLE: X_param_table(cfg, table, n_elems, n_arena, handle)
template <class Cfg, class Table>
int composite_table_size(const Cfg& cfg, int64_t* n_tensors, int64_t* n_elems, Table table_fn) {
  CAPI_TRY
  std::vector<ParamDesc> t;
  int64_t n = 0;
  std::string e = table_fn(cfg, t, &n, nullptr, nullptr);
  if (!e.empty()) return capi_fail(VITX_ERR_INVALID, e);
  if (n_tensors) *n_tensors = (int64_t)t.size();
  if (n_elems) *n_elems = n;
  return VITX_OK;
  CAPI_CATCH
}
template <class Cfg, class Table>
int composite_table_entry(const Cfg& cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank, int64_t* offset_elems, Table table_fn) {
  CAPI_TRY
  std::vector<ParamDesc> t;
  std::string e = table_fn(cfg, t, nullptr, nullptr, nullptr);
  if (!e.empty()) return capi_fail(VITX_ERR_INVALID, e);
  return write_table_entry(t, index, name, name_cap, shape, rank, offset_elems);
  CAPI_CATCH
}
// CREATE: X_create(cfg, &handle, err)
template <class Cfg, class M, class Create>
int composite_create(const Cfg& cfg, M** out, Create create_fn) {
  CAPI_TRY
  std::string err;
  M* m = nullptr;
  int rc = create_fn(cfg, &m, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  *out = m;
  return VITX_OK;
  CAPI_CATCH
}
// host forward: the image (`img_elems` floats each) into m->img, fwd(err) on it, the logits back, synchronised
template <class M, class Fwd>
int composite_forward_host(M* m, const float* img_host, int64_t img_elems, int b, float* logits_host, Fwd fwd) {
  CAPI_TRY
  if (b <= 0 || b > m->cfg.max_batch) return capi_fail(VITX_ERR_INVALID, "batch must be in [1, max_batch]");
  CAPI_HIP(hipMemcpyAsync(m->img, img_host, (size_t)b * img_elems * 4, hipMemcpyHostToDevice, m->stream));
  std::string err;
  int rc = fwd(err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  CAPI_HIP(hipMemcpyAsync(logits_host, m->logits, (size_t)b * m->nc * 4, hipMemcpyDeviceToHost, m->stream));
  CAPI_HIP(hipStreamSynchronize(m->stream));
  return VITX_OK;
  CAPI_CATCH
}
// host backward: dlogits into m->dlogits, bwd(dimg_dev_or_null, err), d(img) back when asked for, synchronised
template <class M, class Bwd>
int composite_backward_host(M* m, const float* dlogits_host, float* dimg_host_or_null, int64_t img_elems, Bwd bwd) {
  CAPI_TRY
  if (!m->have_fwd) return capi_fail(VITX_ERR_STATE, "backward requires a preceding forward");
  CAPI_HIP(hipMemcpyAsync(m->dlogits, dlogits_host, (size_t)m->b * m->nc * 4, hipMemcpyHostToDevice, m->stream));
  std::string err;
  int rc = bwd(dimg_host_or_null ? m->dimg : nullptr, err);
  if (rc != VITX_OK) return capi_fail(rc, err);
  if (dimg_host_or_null) CAPI_HIP(hipMemcpyAsync(dimg_host_or_null, m->dimg, (size_t)m->b * img_elems * 4, hipMemcpyDeviceToHost, m->stream));
  CAPI_HIP(hipStreamSynchronize(m->stream));
  return VITX_OK;
  CAPI_CATCH
}
// the tail of every *_read: n floats at src to the host, refused when they do not fit
inline int composite_read_tail(const float* src, int64_t n, float* out_host, int64_t cap, int64_t* n_elems, hipStream_t stream) {
  if (n_elems) *n_elems = n;
  if (n > cap) return capi_fail(VITX_ERR_INVALID, "output buffer too small");
  CAPI_HIP(hipMemcpyAsync(out_host, src, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
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
