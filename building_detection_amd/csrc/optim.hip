// The optimizers beyond the reference's plain Adam (sg_adam_step, train.hip): AdamW / AMSGrad / SGD with (Nesterov) momentum,
// gradient clipping by value, by per-parameter norm or by global norm, and an exponential moving average of the weights.
//
// Both kernels walk ONE chunk table (sg_optim_table, built once per model on the host): a chunk is a 16-byte aligned run of at
// most 4 Ki elements of ONE parameter, so a workgroup never touches the padding between two parameters of the arena
// and everything that differs from parameter to parameter (decayed or not, its clip scale) is uniform in a workgroup.
//   sg_optim_grad_norms   sum (grad_scale * g)^2 per chunk in fp64 (block tree, fixed order), then two small kernels fold the
//                         chunk sums per parameter and the parameter sums, each in a fixed order: no float atomics, the same
//                         bits in every run.
//   sg_optim_step         one streaming pass: 16-byte loads and stores of w, g and the state arenas the configuration has,
//                         scalar code only for the last 1..3 elements of a parameter.  The clip scale comes from the norm buffer
//                         and the step's learning rates from arguments or from device memory (a captured step): no host sync.
#include "sg_reduce.h"

namespace {

constexpr int OPT_THREADS = 256;
// Workgroups.  Chunks differ in length (most parameters are far shorter than the host's bound of 4 Ki elements = 4 trips of a
// workgroup); up to the cap there is one workgroup per chunk, a longer table takes further trips of the chunk loop.  Measured on
// DeepLabv3+'s 64.5 M elements, AdamW alone against sg_adam_step's 364 us in the same run: 369 / 356 / 371 / 434 / 474 us at chunk
// bounds of 1 / 4 / 16 / 64 / 256 Ki elements (LAB_NOTEBOOK 31): long chunks leave the last workgroups running alone.
constexpr int OPT_GRID_CAP = 8192;
constexpr int OPT_MAX_CHUNK = 1 << 20;    // elements: what a table may ask of one workgroup trip

// fixed-order sum of one double per thread of a 256-thread workgroup; valid in every thread
__device__ __forceinline__ double block_sum_f64(double v, double* sm) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();  // the previous trip's readers are done with sm
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__device__ __forceinline__ double sq_add(double acc, const f32x4 gv, double gsd) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = (double)gv[k] * gsd;
    acc += d * d;
  }
  return acc;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_part_kernel(const sg_optim_chunk* __restrict__ chunks, int nchunks,
                                                                      const float* __restrict__ g, float gs,
                                                                      double* __restrict__ part) {
  __shared__ double sm[4];
  const double gsd = (double)gs;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const sg_optim_chunk ch = chunks[c];
    const float* __restrict__ gp = g + ch.start;
    const int nv = ch.length >> 2;
    double acc = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * OPT_THREADS < nv; i += 4 * OPT_THREADS) {   // four loads in flight; the sum keeps the order of the plain loop
      f32x4 gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = reinterpret_cast<const f32x4*>(gp)[i + u * OPT_THREADS];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = sq_add(acc, gv[u], gsd);
    }
    for (; i < nv; i += OPT_THREADS) acc = sq_add(acc, reinterpret_cast<const f32x4*>(gp)[i], gsd);
    const int t = (nv << 2) + (int)threadIdx.x;   // the parameter's last 1..3 elements
    if (t < ch.length) {
      const double d = (double)gp[t] * gsd;
      acc += d * d;
    }
    const double s = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) part[c] = s;
  }
}

// norms[1 + s] = the chunk sums of segment s: one wave per segment, lane l adds chunks l, l + 64, ... of the segment in that
// order, then the fixed shuffle tree.  (One thread per segment walking its chunks one after the other - up to 200 of them, each
// add waiting for a load from another XCD's L2 - was the larger part of the norm pass's time.)
__global__ __launch_bounds__(OPT_THREADS) void optim_norm_seg_kernel(const sg_optim_seg* __restrict__ segs, int nseg,
                                                                     const double* __restrict__ part,
                                                                     double* __restrict__ norms) {
  const int s = blockIdx.x * (OPT_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= nseg) return;
  const sg_optim_seg sg = segs[s];
  double a = 0.0;
  for (int c = sg.chunk_begin + lane; c < sg.chunk_end; c += 64) a += part[c];
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  if (lane == 0) norms[1 + s] = a;
}

// norms[0] = the segment sums: thread t adds segments t, t + 256, ... in that order, then the fixed block tree
__global__ __launch_bounds__(OPT_THREADS) void optim_norm_total_kernel(int nseg, double* __restrict__ norms) {
  __shared__ double sm[4];
  double tot = 0.0;
  for (int s = threadIdx.x; s < nseg; s += OPT_THREADS) tot += norms[1 + s];
  const double t = block_sum_f64(tot, sm);
  if (threadIdx.x == 0) norms[0] = t;
}

enum { K_ADAM = 0, K_SGD = 1, K_SGDM = 2 };   // the update's form: SGD without / with a momentum arena

struct StepArgs {
  const sg_optim_chunk* chunks;
  const sg_optim_seg* segs;
  int nchunks;
  float* w;
  const float* g;
  float *m, *v, *vhat, *ema;
  const double* norms;
  const float* lr_dev;   // {lr_t, lr} in device memory, or nullptr: the two arguments below
  float lr_t, lr;
  float b1, b2, eps, mu, wd, clip_c, ema_mom, gs;
  int clip, nesterov;
};

// what is uniform in one chunk
struct ChunkP {
  float lr_t, lr, lrwd, scale;
};

template <int KIND, bool AMS, bool EMA>
__device__ __forceinline__ void update1(const StepArgs& a, const ChunkP& q, float& w, float g, float& m, float& v, float& vh,
                                        float& e) {
  float gk = g * a.gs;
  if (a.clip == SG_OPT_CLIP_VALUE) gk = gk > a.clip_c ? a.clip_c : (gk < -a.clip_c ? -a.clip_c : gk);   // a NaN stays a NaN
  else if (a.clip != SG_OPT_CLIP_NONE) gk *= q.scale;
  w -= q.lrwd * w;
  if constexpr (KIND == K_ADAM) {
    m = a.b1 * m + (1.f - a.b1) * gk;
    v = a.b2 * v + (1.f - a.b2) * gk * gk;
    float d = v;
    if constexpr (AMS) {
      vh = fmaxf(vh, v);
      d = vh;
    }
    w -= q.lr_t * m / (sqrtf(d) + a.eps);
  } else if constexpr (KIND == K_SGDM) {
    m = a.mu * m - q.lr * gk;
    w += a.nesterov ? a.mu * m - q.lr * gk : m;
  } else {
    w -= q.lr * gk;
  }
  if constexpr (EMA) e = a.ema_mom * e + (1.f - a.ema_mom) * w;
}

template <int KIND, bool AMS, bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const StepArgs a) {
  ChunkP q;
  q.lr_t = a.lr_dev ? a.lr_dev[0] : a.lr_t;
  q.lr = a.lr_dev ? a.lr_dev[1] : a.lr;
  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const sg_optim_chunk ch = a.chunks[c];
    q.lrwd = (a.segs[ch.segment].flags & SG_OPT_SEG_DECAY) ? q.lr * a.wd : 0.f;
    q.scale = 1.f;
    if (a.clip == SG_OPT_CLIP_NORM || a.clip == SG_OPT_CLIP_GLOBAL) {
      const float nrm = (float)sqrt(a.norms[a.clip == SG_OPT_CLIP_GLOBAL ? 0 : 1 + ch.segment]);
      q.scale = a.clip_c / fmaxf(nrm, a.clip_c);
    }
    float* __restrict__ wp = a.w + ch.start;
    const float* __restrict__ gp = a.g + ch.start;
    float* __restrict__ mp = KIND != K_SGD ? a.m + ch.start : nullptr;
    float* __restrict__ vp = KIND == K_ADAM ? a.v + ch.start : nullptr;
    float* __restrict__ hp = AMS ? a.vhat + ch.start : nullptr;
    float* __restrict__ ep = EMA ? a.ema + ch.start : nullptr;
    const int nv = ch.length >> 2;
    for (int i = threadIdx.x; i < nv; i += OPT_THREADS) {
      f32x4 wv = reinterpret_cast<f32x4*>(wp)[i], mv = {0.f, 0.f, 0.f, 0.f}, vv = mv, hv = mv, ev = mv;
      const f32x4 gv = reinterpret_cast<const f32x4*>(gp)[i];
      if constexpr (KIND != K_SGD) mv = reinterpret_cast<f32x4*>(mp)[i];
      if constexpr (KIND == K_ADAM) vv = reinterpret_cast<f32x4*>(vp)[i];
      if constexpr (AMS) hv = reinterpret_cast<f32x4*>(hp)[i];
      if constexpr (EMA) ev = reinterpret_cast<f32x4*>(ep)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float w1 = wv[k], m1 = mv[k], v1 = vv[k], h1 = hv[k], e1 = ev[k];
        update1<KIND, AMS, EMA>(a, q, w1, gv[k], m1, v1, h1, e1);
        wv[k] = w1; mv[k] = m1; vv[k] = v1; hv[k] = h1; ev[k] = e1;
      }
      reinterpret_cast<f32x4*>(wp)[i] = wv;
      if constexpr (KIND != K_SGD) reinterpret_cast<f32x4*>(mp)[i] = mv;
      if constexpr (KIND == K_ADAM) reinterpret_cast<f32x4*>(vp)[i] = vv;
      if constexpr (AMS) reinterpret_cast<f32x4*>(hp)[i] = hv;
      if constexpr (EMA) reinterpret_cast<f32x4*>(ep)[i] = ev;
    }
    const int t = (nv << 2) + (int)threadIdx.x;   // the parameter's last 1..3 elements
    if (t < ch.length) {
      float w1 = wp[t], m1 = 0.f, v1 = 0.f, h1 = 0.f, e1 = 0.f;
      if constexpr (KIND != K_SGD) m1 = mp[t];
      if constexpr (KIND == K_ADAM) v1 = vp[t];
      if constexpr (AMS) h1 = hp[t];
      if constexpr (EMA) e1 = ep[t];
      update1<KIND, AMS, EMA>(a, q, w1, gp[t], m1, v1, h1, e1);
      wp[t] = w1;
      if constexpr (KIND != K_SGD) mp[t] = m1;
      if constexpr (KIND == K_ADAM) vp[t] = v1;
      if constexpr (AMS) hp[t] = h1;
      if constexpr (EMA) ep[t] = e1;
    }
  }
}

// The host copy of a table: every chunk 16-byte aligned, non-empty, inside the arena, behind its predecessor; the segments'
// chunk ranges tile [0, nchunks) in order and every chunk names the segment whose range holds it.
bool table_ok(const sg_optim_table* t, const char* who) {
  if (!t || !t->chunks || !t->segs || !t->chunks_dev || !t->segs_dev || t->nchunks <= 0 || t->nseg <= 0 || t->n <= 0) {
    sg_set_error("%s: empty or null table", who);
    return false;
  }
  int64_t end = 0;
  int c = 0;
  for (int s = 0; s < t->nseg; ++s) {
    const sg_optim_seg& sg = t->segs[s];
    if (sg.chunk_begin != c || sg.chunk_end <= sg.chunk_begin || sg.chunk_end > t->nchunks) {
      sg_set_error("%s: segment %d holds chunks [%d, %d), expected to start at %d of %d", who, s, sg.chunk_begin, sg.chunk_end, c,
                   t->nchunks);
      return false;
    }
    for (; c < sg.chunk_end; ++c) {
      const sg_optim_chunk& ch = t->chunks[c];
      if (ch.segment != s || (ch.start & 3) || ch.start < end || ch.length <= 0 || ch.length > OPT_MAX_CHUNK ||
          ch.start + ch.length > t->n) {
        sg_set_error("%s: chunk %d = (start %lld, length %d, segment %d) in segment %d of an arena of %lld", who, c,
                     (long long)ch.start, ch.length, ch.segment, s, (long long)t->n);
        return false;
      }
      end = ch.start + ch.length;
    }
  }
  if (c != t->nchunks) {
    sg_set_error("%s: %d of %d chunks belong to no segment", who, t->nchunks - c, t->nchunks);
    return false;
  }
  return true;
}

unsigned table_grid(const sg_optim_table* t) { return (unsigned)(t->nchunks < OPT_GRID_CAP ? t->nchunks : OPT_GRID_CAP); }

template <int KIND, bool AMS, bool EMA>
void launch_step(const sg_optim_table* t, hipStream_t stream, const StepArgs& a) {
  hipLaunchKernelGGL((optim_step_kernel<KIND, AMS, EMA>), dim3(table_grid(t)), dim3(OPT_THREADS), 0, stream, a);
}

template <int KIND>
void launch_step_kind(const sg_optim_table* t, hipStream_t stream, const StepArgs& a, bool ams, bool ema) {
  if (ams && ema) launch_step<KIND, true, true>(t, stream, a);
  else if (ams) launch_step<KIND, true, false>(t, stream, a);
  else if (ema) launch_step<KIND, false, true>(t, stream, a);
  else launch_step<KIND, false, false>(t, stream, a);
}

bool finite_nonneg(float v) { return v >= 0.f && v <= 3.4e38f; }

}  // namespace

size_t sg_optim_norms_ws_bytes(int32_t nchunks) { return nchunks > 0 ? (size_t)nchunks * sizeof(double) : 0; }

int sg_optim_grad_norms(sg_ctx* ctx, void* stream, const sg_optim_table* table, const void* g, float grad_scale, void* norms,
                        void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && g && norms && ws, "sg_optim_grad_norms: bad argument");
  if (!table_ok(table, "sg_optim_grad_norms")) return SG_EINVAL;
  SG_CHECK_ARG(sg_aligned16(g) && sg_aligned16(norms) && sg_aligned16(ws),
               "sg_optim_grad_norms: the arena, the norm buffer and the workspace must be 16-byte aligned");
  if (ws_bytes < sg_optim_norms_ws_bytes(table->nchunks)) {
    sg_set_error("sg_optim_grad_norms: workspace %zu < %zu bytes", ws_bytes, sg_optim_norms_ws_bytes(table->nchunks));
    return SG_EWORKSPACE;
  }
  hipLaunchKernelGGL(optim_norm_part_kernel, dim3(table_grid(table)), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                     (const sg_optim_chunk*)table->chunks_dev, table->nchunks, (const float*)g, grad_scale, (double*)ws);
  SG_LAUNCH_CHECK("optim_norm_part_kernel");
  hipLaunchKernelGGL(optim_norm_seg_kernel, dim3((unsigned)sg_cdiv(table->nseg, OPT_THREADS / 64)), dim3(OPT_THREADS), 0,
                     (hipStream_t)stream, (const sg_optim_seg*)table->segs_dev, table->nseg, (const double*)ws, (double*)norms);
  SG_LAUNCH_CHECK("optim_norm_seg_kernel");
  hipLaunchKernelGGL(optim_norm_total_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, table->nseg, (double*)norms);
  SG_LAUNCH_CHECK("optim_norm_total_kernel");
  return 0;
}

int sg_optim_step(sg_ctx* ctx, void* stream, const sg_optim_desc* d, const sg_optim_table* table, void* w, const void* g, void* m,
                  void* v, void* vhat, void* ema, const void* norms, float lr_t, float lr, const void* lr_dev) {
  SG_CHECK_ARG(ctx && d && w && g, "sg_optim_step: bad argument");
  SG_CHECK_ARG(d->kind == SG_OPT_ADAM || d->kind == SG_OPT_SGD, "sg_optim_step: kind %d", d->kind);
  SG_CHECK_ARG(!(d->flags & ~(SG_OPT_AMSGRAD | SG_OPT_NESTEROV | SG_OPT_EMA)), "sg_optim_step: flags 0x%x", d->flags);
  SG_CHECK_ARG(d->clip >= SG_OPT_CLIP_NONE && d->clip <= SG_OPT_CLIP_GLOBAL, "sg_optim_step: clip mode %d", d->clip);
  const bool adam = d->kind == SG_OPT_ADAM, ams = adam && (d->flags & SG_OPT_AMSGRAD), use_ema = d->flags & SG_OPT_EMA;
  const bool mom = !adam && d->momentum != 0.f, by_norm = d->clip == SG_OPT_CLIP_NORM || d->clip == SG_OPT_CLIP_GLOBAL;
  SG_CHECK_ARG(adam || !(d->flags & SG_OPT_AMSGRAD), "sg_optim_step: amsgrad belongs to Adam");
  SG_CHECK_ARG(!adam || !(d->flags & SG_OPT_NESTEROV), "sg_optim_step: nesterov belongs to SGD");
  SG_CHECK_ARG(finite_nonneg(d->beta1) && finite_nonneg(d->beta2) && finite_nonneg(d->eps) && finite_nonneg(d->momentum) &&
                   finite_nonneg(d->weight_decay) && finite_nonneg(d->clip_c) && finite_nonneg(d->ema_momentum) &&
                   finite_nonneg(d->grad_scale),
               "sg_optim_step: a negative or non-finite hyperparameter");
  SG_CHECK_ARG(d->clip == SG_OPT_CLIP_NONE || d->clip_c > 0.f, "sg_optim_step: clip mode %d needs a positive constant", d->clip);
  SG_CHECK_ARG((!adam && !mom) || m, "sg_optim_step: this configuration needs the moment arena m");
  SG_CHECK_ARG(!adam || v, "sg_optim_step: Adam needs the moment arena v");
  SG_CHECK_ARG(!ams || vhat, "sg_optim_step: amsgrad needs the arena vhat");
  SG_CHECK_ARG(!use_ema || ema, "sg_optim_step: the weight average needs its arena");
  SG_CHECK_ARG(!by_norm || norms, "sg_optim_step: clipping by norm needs the buffer sg_optim_grad_norms wrote");
  if (!table_ok(table, "sg_optim_step")) return SG_EINVAL;
  SG_CHECK_ARG(sg_aligned16(w) && sg_aligned16(g) && sg_aligned16(m) && sg_aligned16(v) && sg_aligned16(vhat) &&
                   sg_aligned16(ema) && sg_aligned16(norms),
               "sg_optim_step: the arenas and the norm buffer must be 16-byte aligned");
  StepArgs a;
  a.chunks = (const sg_optim_chunk*)table->chunks_dev;
  a.segs = (const sg_optim_seg*)table->segs_dev;
  a.nchunks = table->nchunks;
  a.w = (float*)w;
  a.g = (const float*)g;
  a.m = (float*)m;
  a.v = (float*)v;
  a.vhat = (float*)vhat;
  a.ema = (float*)ema;
  a.norms = (const double*)norms;
  a.lr_dev = (const float*)lr_dev;
  a.lr_t = lr_t;
  a.lr = lr;
  a.b1 = d->beta1; a.b2 = d->beta2; a.eps = d->eps; a.mu = d->momentum; a.wd = d->weight_decay; a.clip_c = d->clip_c;
  a.ema_mom = d->ema_momentum; a.gs = d->grad_scale;
  a.clip = d->clip;
  a.nesterov = (d->flags & SG_OPT_NESTEROV) ? 1 : 0;
  if (adam) launch_step_kind<K_ADAM>(table, (hipStream_t)stream, a, ams, use_ema);
  else if (mom) launch_step_kind<K_SGDM>(table, (hipStream_t)stream, a, false, use_ema);
  else launch_step_kind<K_SGD>(table, (hipStream_t)stream, a, false, use_ema);
  SG_LAUNCH_CHECK("optim_step_kernel");
  return 0;
}
