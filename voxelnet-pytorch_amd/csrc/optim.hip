// Optimizer tail of the train step (train.py:153-154): clip_grad_norm_(parameters, max_norm) followed by the update of
// one of two rules, as TWO launches over a chunk table instead of torch's multi-tensor / elementwise launches over the
// 104 parameter tensors.
//   total = sqrt(sum_i |g_i|^2);  coef = min(1, max_norm / (total + 1e-6));  g' = g * coef
//   vn_clip_sgd    plain SGD (train.py:130: SGD(lr), no momentum, no weight decay):   p -= lr * g'
//   vn_clip_adamw  torch.optim.AdamW's single-tensor update (torch/optim/adam.py, _single_tensor_adam with decoupled
//                  weight decay, amsgrad = False, maximize = False; what SECOND, PointPillars and what followed train with):
//                    p *= 1 - lr * wd;  m += (g' - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g'^2
//                    p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// The chunk table (device memory, built once by the caller for a fixed set of tensors) cuts every tensor tuple into
// pieces of at most VN_OPT_CHUNK elements; one workgroup per chunk in both kernels.  The clip is ONE piece of code for
// both rules: k_clip_sumsq, and the head and the chunk walk of k_clip_update; a rule (SgdRule, AdamRule) is a plain struct
// in the kernel arguments that names its chunk type and supplies
//   aligned(c)     whether all of the chunk's pointers allow 16-byte accesses,
//   bind(c)        what the chunk's elements share (SGD: lr; AdamW: the chunk's hyperparameter slot), taken once per chunk,
//   apply<V>(...)  load, update and store element i as V = float4 or V = float.
// Every AdamW chunk names one of at most VN_OPT_MAX_SLOTS hyperparameter slots (parameter group x step count); the slots'
// scalars are worked out in double on the host at every call and travel in the kernel arguments, so a scheduler's new lr
// or beta1 costs no device table rebuild and no copy.
// HBM-bound: 4 B read per element in the first pass; in the second 12 B for SGD (g read, p read+write) and 28 B for AdamW
// (g, p, m, v read; p, m, v written), +4 when the scaled gradients are written back.
// Weight average: ema = lerp(ema, p, w), w = 1 - decay by value.  Each rule has an Ema flavour (vn_clip_sgd_ema,
// vn_clip_adamw_ema) whose chunks carry the shadow's pointer and whose apply<V> averages the parameter it has just computed:
// +8 B per element in the second launch (20 B SGD, 36 B AdamW) against 12 B and a launch for a pass of its own; k_clip_sumsq
// and the head of k_clip_update are the same code.  vn_ema_update (k_ema_update) is that pass, for what no rule touches.
// Sums: fp32 per thread -> one fp32 partial per chunk -> every workgroup of the second kernel adds the partials in
// double in the same fixed order (deterministic, no atomics, no third launch).
#include "common.h"

#include <charconv>
#include <cmath>
#include <type_traits>

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = 4096;           // == VN_OPT_CHUNK in the header
static_assert(OPT_CHUNK == VN_OPT_CHUNK, "header and kernel disagree on the chunk size");

template <class... P> __device__ __forceinline__ bool aligned16(const P *...p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// f on one element, or on each of a float4's four in turn
template <class F, class... T> __device__ __forceinline__ void per_lane(F f, float &a, T &...r) { f(a, r...); }
template <class F, class... T> __device__ __forceinline__ void per_lane(F f, float4 &a, T &...r) {
    f(a.x, r.x...); f(a.y, r.y...); f(a.z, r.z...); f(a.w, r.w...);
}

template <class Chunk>
__global__ void __launch_bounds__(OPT_THREADS) k_clip_sumsq(const Chunk *__restrict__ chunks, float *__restrict__ partial) {
    const Chunk c = chunks[blockIdx.x];
    const float *__restrict__ g = c.grad;
    float s = 0.f;
    if (aligned16(g)) {
        const int n4 = c.n >> 2;
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
            const float4 v = reinterpret_cast<const float4 *>(g)[i];
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < c.n; i += OPT_THREADS) s += g[i] * g[i];
    } else {
        for (int i = threadIdx.x; i < c.n; i += OPT_THREADS) s += g[i] * g[i];
    }
    __shared__ float red[OPT_THREADS / 64];
    s = vn_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < OPT_THREADS / 64; ++w) t += red[w];
        partial[blockIdx.x] = t;
    }
}

template <class Rule>
__global__ void __launch_bounds__(OPT_THREADS) k_clip_update(const typename Rule::Chunk *__restrict__ chunks, int n_chunks,
                                                            const float *__restrict__ partial, float max_norm,
                                                            const Rule rule, int scale_grads, float *__restrict__ total_norm) {
    // every workgroup recomputes the (same) total from the partials: n_chunks * 4 B from L2
    double s = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += OPT_THREADS) s += (double)partial[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double red[OPT_THREADS / 64];
    __shared__ float coef_s;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < OPT_THREADS / 64; ++w) t += red[w];
        const float total = (float)sqrt(t);
        const float coef = max_norm / (total + 1e-6f);         // torch.nn.utils.clip_grad_norm_
        coef_s = coef < 1.f ? coef : 1.f;                        // clamp(max=1.0); NaN stays NaN as in torch
        if (coef != coef) coef_s = coef;
        if (blockIdx.x == 0 && total_norm) *total_norm = total;
    }
    __syncthreads();
    const float coef = coef_s;
    const typename Rule::Chunk c = chunks[blockIdx.x];
    const auto h = rule.bind(c);
    // 16-byte accesses plus the chunk's tail, or element by element when a pointer is off a 16-byte boundary (a tensor
    // inside a flat buffer)
    if (Rule::aligned(c)) {
        const int n4 = c.n >> 2;
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) rule.template apply<float4>(c, i, coef, h, scale_grads);
        for (int i = (n4 << 2) + threadIdx.x; i < c.n; i += OPT_THREADS) rule.template apply<float>(c, i, coef, h, scale_grads);
    } else {
        for (int i = threadIdx.x; i < c.n; i += OPT_THREADS) rule.template apply<float>(c, i, coef, h, scale_grads);
    }
}

// lerp(a, b, w) = a + w * (b - a) with the roundings of torch's device kernel for lerp_: contracted, and the other form
// from weight 0.5 on.  AdamW's exp_avg and the weight average (vn_ema_update, the Ema rules) are this one function.
__device__ __forceinline__ float lerp_element(float a, float b, float w) {
    const float d = b - a;
    return w < 0.5f ? fmaf(w, d, a) : fmaf(-d, 1.f - w, b);
}

// The Ema flavour of a rule: its chunk carries one more pointer, its kernel argument one more float (the average's
// weight), and apply<V> averages the parameter value it holds in a register into the shadow: one load and one store more.
// A NULL shadow (device data, looked at per chunk) leaves the average out.  The plain flavour has neither the member nor
// the code: its instantiations are what they were before the average existed.
template <bool Ema> struct EmaWeight {};
template <> struct EmaWeight<true> { float ema_w; };

template <class V> __device__ __forceinline__ void ema_store(float *ema, int i, const V &pv, float w) {
    if (!ema) return;
    V *__restrict__ e = reinterpret_cast<V *>(ema);
    V ev = e[i], xv = pv;
    per_lane([=](float &e1, float &x1) { e1 = lerp_element(e1, x1, w); }, ev, xv);
    e[i] = ev;
}

template <bool Ema> struct SgdRuleT : EmaWeight<Ema> {
    using Chunk = std::conditional_t<Ema, vnParamChunkEma, vnParamChunk>;
    float lr;
    __device__ float bind(const Chunk &) const { return lr; }
    static __device__ bool aligned(const Chunk &c) {
        if constexpr (Ema) return aligned16(c.param, c.grad, c.ema);
        else return aligned16(c.param, c.grad);
    }
    template <class V> __device__ void apply(const Chunk &c, int i, float coef, float lr, int scale_grads) const {
        V *__restrict__ p = reinterpret_cast<V *>(c.param);
        V *__restrict__ g = reinterpret_cast<V *>(c.grad);
        V gv = g[i], pv = p[i];
        per_lane([=](float &g1, float &p1) { g1 *= coef; p1 -= lr * g1; }, gv, pv);
        p[i] = pv;
        if (scale_grads) g[i] = gv;
        if constexpr (Ema) ema_store<V>(c.ema, i, pv, this->ema_w);
    }
};
using SgdRule = SgdRuleT<false>;

struct AdamSlotK {          // one slot as the kernel wants it
    float neg_step_size;    // -lr / (1 - beta1^t)
    float decay;            // 1 - lr * wd
    float omb1;             // 1 - beta1
    float beta2, omb2;      // beta2, 1 - beta2
    float inv_bc2_sqrt;     // 1 / (float)sqrt(1 - beta2^t), the reciprocal taken in float as torch's division by a scalar does
    float eps;
};

// one element: g is scaled in place (the caller stores it when scale_grads is set).  The roundings are those of torch's
// device kernels for the same update, one kernel per line there: mul_ | lerp_ (a + w * (b - a), contracted; the other
// form from weight 0.5 on) | mul_, addcmul_ (a + alpha * b * c, the last product contracted into the sum) | sqrt, a
// division by a scalar done as a product with its float reciprocal, add_ | addcdiv_ (a + alpha * (b / c), contracted).  The
// build has contraction off (Makefile), hence the explicit fmaf.  Measured against torch on the MI355X: exp_avg comes out
// equal bit for bit (unclipped gradients), exp_avg_sq and p still differ in the last bit for a part of the elements
// (DESIGN.md section 1d); what this buys is the whole detector's second step, whose gradient norm equals the torch tail's
// bit for bit with this form and was 1.9e-4 off with the uncontracted one.
__device__ __forceinline__ void adam_element(float &p, float &g, float &m, float &v, float coef, const AdamSlotK &h) {
    g *= coef;
    p *= h.decay;
    m = lerp_element(m, g, h.omb1);
    v = fmaf(h.omb2 * g, g, h.beta2 * v);
    const float denom = sqrtf(v) * h.inv_bc2_sqrt + h.eps;
    p = fmaf(h.neg_step_size, m / denom, p);
}

template <bool Ema> struct AdamRuleT : EmaWeight<Ema> {
    using Chunk = std::conditional_t<Ema, vnAdamChunkEma, vnAdamChunk>;
    AdamSlotK slot[VN_OPT_MAX_SLOTS];
    int n_slots;
    // the slot index is device data: clamped, never trusted
    __device__ AdamSlotK bind(const Chunk &c) const { return slot[c.slot < 0 ? 0 : (c.slot >= n_slots ? n_slots - 1 : c.slot)]; }
    static __device__ bool aligned(const Chunk &c) {
        if constexpr (Ema) return aligned16(c.param, c.grad, c.exp_avg, c.exp_avg_sq, c.ema);
        else return aligned16(c.param, c.grad, c.exp_avg, c.exp_avg_sq);
    }
    template <class V> __device__ void apply(const Chunk &c, int i, float coef, const AdamSlotK &h, int scale_grads) const {
        V *__restrict__ p = reinterpret_cast<V *>(c.param);
        V *__restrict__ g = reinterpret_cast<V *>(c.grad);
        V *__restrict__ m = reinterpret_cast<V *>(c.exp_avg);
        V *__restrict__ v = reinterpret_cast<V *>(c.exp_avg_sq);
        V gv = g[i], pv = p[i], mv = m[i], vv = v[i];
        per_lane([&](float &p1, float &g1, float &m1, float &v1) { adam_element(p1, g1, m1, v1, coef, h); }, pv, gv, mv, vv);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
        if (scale_grads) g[i] = gv;
        if constexpr (Ema) ema_store<V>(c.ema, i, pv, this->ema_w);
    }
};
using AdamRule = AdamRuleT<false>;

// the average alone: one workgroup per (source, shadow) piece
__global__ void __launch_bounds__(OPT_THREADS) k_ema_update(const vnEmaChunk *__restrict__ chunks, float w) {
    const vnEmaChunk c = chunks[blockIdx.x];
    if (!c.src || !c.ema) return;
    const float *__restrict__ x = c.src;
    if (aligned16(c.src, c.ema)) {
        const int n4 = c.n >> 2;
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) ema_store<float4>(c.ema, i, reinterpret_cast<const float4 *>(x)[i], w);
        for (int i = (n4 << 2) + threadIdx.x; i < c.n; i += OPT_THREADS) ema_store<float>(c.ema, i, x[i], w);
    } else {
        for (int i = threadIdx.x; i < c.n; i += OPT_THREADS) ema_store<float>(c.ema, i, x[i], w);
    }
}

size_t workspace_bytes(int32_t n_chunks) {      // one fp32 partial per chunk
    if (n_chunks <= 0) return 0;
    return vn_align(sizeof(float) * (size_t)n_chunks);
}

// the tail both entry points share: argument checks, then the workspace, then the two launches
template <class Rule>
int clip_update(const typename Rule::Chunk *chunks, int32_t n_chunks, float max_norm, const Rule &rule, int32_t scale_grads,
                void *workspace, size_t ws_bytes, float *total_norm, vnStream stream) {
    VN_CHECK_ARG(chunks && n_chunks > 0 && workspace && max_norm > 0.f);
    if (ws_bytes < workspace_bytes(n_chunks)) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    float *partial = static_cast<float *>(workspace);
    k_clip_sumsq<<<n_chunks, OPT_THREADS, 0, st>>>(chunks, partial);
    VN_LAUNCH_STATUS();
    k_clip_update<<<n_chunks, OPT_THREADS, 0, st>>>(chunks, n_chunks, partial, max_norm, rule, scale_grads, total_norm);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

// The ABI carries the hyperparameters as floats; the caller meant a decimal (0.9, 0.999, 1e-8).  (double)0.999f is
// 0.99900001287..., whose 1 - beta2 is off by 1.3e-5 of itself — far above the rounding of the update.  The shortest
// decimal form that rounds to the float (std::to_chars) read back as a double gives 0.999 again; a value that needs all
// of a double's digits loses at most half a float ulp, as any float would.
double widen(float x) {
    char buf[32];
    const std::to_chars_result r = std::to_chars(buf, buf + sizeof(buf), x);
    double d = (double)x;
    if (r.ec == std::errc()) std::from_chars(buf, r.ptr, d);
    return d;
}

// vnAdamHyper -> the rule's slots (checks first; the scalars in double, see widen)
template <class Rule> int adam_slots(const vnAdamHyper *hyper, Rule &rule) {
    VN_CHECK_ARG(hyper && hyper->n_slots >= 1 && hyper->n_slots <= VN_OPT_MAX_SLOTS);
    rule.n_slots = hyper->n_slots;
    for (int i = 0; i < hyper->n_slots; ++i) {
        const vnAdamSlot &s = hyper->slot[i];
        // (written so that a NaN fails every test)
        VN_CHECK_ARG(s.beta1 >= 0.f && s.beta1 < 1.f && s.beta2 >= 0.f && s.beta2 < 1.f);
        VN_CHECK_ARG(s.eps >= 0.f && s.lr >= 0.f && s.weight_decay >= 0.f && s.step >= 1);
        const double lr = widen(s.lr), b1 = widen(s.beta1), b2 = widen(s.beta2), wd = widen(s.weight_decay);
        const double bc1 = 1.0 - std::pow(b1, (double)s.step), bc2 = 1.0 - std::pow(b2, (double)s.step);
        AdamSlotK &k = rule.slot[i];
        k.neg_step_size = (float)(-(lr / bc1));
        k.decay = (float)(1.0 - lr * wd);
        k.omb1 = (float)(1.0 - b1);
        k.beta2 = (float)b2;
        k.omb2 = (float)(1.0 - b2);
        k.inv_bc2_sqrt = 1.f / (float)std::sqrt(bc2);
        k.eps = s.eps;
    }
    return VN_OK;
}

}  // namespace

extern "C" size_t vn_clip_sgd_workspace_bytes(int32_t n_chunks) { return workspace_bytes(n_chunks); }
extern "C" size_t vn_clip_adamw_workspace_bytes(int32_t n_chunks) { return workspace_bytes(n_chunks); }

extern "C" int vn_clip_sgd(const vnParamChunk *chunks, int32_t n_chunks, float max_norm, float lr, int32_t scale_grads,
                           void *workspace, size_t workspace_bytes, float *total_norm, vnStream stream) {
    SgdRule rule = {};
    rule.lr = lr;
    return clip_update(chunks, n_chunks, max_norm, rule, scale_grads, workspace, workspace_bytes, total_norm, stream);
}

extern "C" int vn_clip_sgd_ema(const vnParamChunkEma *chunks, int32_t n_chunks, float max_norm, float lr, int32_t scale_grads,
                               float ema_weight, void *workspace, size_t workspace_bytes, float *total_norm, vnStream stream) {
    VN_CHECK_ARG(ema_weight >= 0.f && ema_weight <= 1.f);          // (a NaN fails both)
    SgdRuleT<true> rule = {};
    rule.lr = lr;
    rule.ema_w = ema_weight;
    return clip_update(chunks, n_chunks, max_norm, rule, scale_grads, workspace, workspace_bytes, total_norm, stream);
}

extern "C" int vn_ema_update(const vnEmaChunk *chunks, int32_t n_chunks, float weight, vnStream stream) {
    VN_CHECK_ARG(chunks && n_chunks > 0 && weight >= 0.f && weight <= 1.f);
    k_ema_update<<<n_chunks, OPT_THREADS, 0, vn_stream(stream)>>>(chunks, weight);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_clip_adamw(const vnAdamChunk *chunks, int32_t n_chunks, const vnAdamHyper *hyper, float max_norm,
                             int32_t scale_grads, void *workspace, size_t workspace_bytes, float *total_norm,
                             vnStream stream) {
    AdamRule rule = {};
    if (const int st = adam_slots(hyper, rule)) return st;
    return clip_update(chunks, n_chunks, max_norm, rule, scale_grads, workspace, workspace_bytes, total_norm, stream);
}

extern "C" int vn_clip_adamw_ema(const vnAdamChunkEma *chunks, int32_t n_chunks, const vnAdamHyper *hyper, float max_norm,
                                 int32_t scale_grads, float ema_weight, void *workspace, size_t workspace_bytes,
                                 float *total_norm, vnStream stream) {
    VN_CHECK_ARG(ema_weight >= 0.f && ema_weight <= 1.f);          // (a NaN fails both)
    AdamRuleT<true> rule = {};
    rule.ema_w = ema_weight;
    if (const int st = adam_slots(hyper, rule)) return st;
    return clip_update(chunks, n_chunks, max_norm, rule, scale_grads, workspace, workspace_bytes, total_norm, stream);
}
