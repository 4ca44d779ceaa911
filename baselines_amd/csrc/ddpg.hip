// DDPG (ddpg/ddpg_learner.py, ddpg/memory.py, ddpg/models.py): the fused train step, the act side, the replay store, the
// parameter-space noise.  Paths in comments are relative to the reference's baselines/.
//
// Design (DESIGN.md "DDPG"): one train step is a chain of about ten dependent GEMM-lets of a few hundred kFLOP each at the
// default shape (B = 64, 2 x 64 tanh).  As separate launches it is pure latency (a dependent boundary costs ~1.5 us), so the
// whole step runs in ONE workgroup of 1024 threads (16 waves, one CU): every phase hands its result to the next through a
// workgroup barrier, activations live in a global workspace (L2/L1-resident at these sizes), arithmetic is fp32 VALU FMA.
// No grid-wide synchronisation exists anywhere in this file.
#include "common.hip.h"

using namespace mrl;

namespace {

constexpr int MAXL = 4;
constexpr int TRAIN_THREADS = 1024;
constexpr int ACT_THREADS = 256;
constexpr int ACT_ROWS = 32;           // rows of one act workgroup
constexpr float LN_EPS = 1e-12f;       // tf.contrib.layers.layer_norm -> tf.nn.batch_normalization variance_epsilon

// flat parameter layout of one network in TF creation order (ddpg/models.py:27-51, common/models.py:75-103):
//   mlp_fc<i>/w [nin][nh], mlp_fc<i>/b [nh], (LayerNorm[_i]/beta [nh], LayerNorm[_i]/gamma [nh]) per layer, then
//   dense/kernel|bias (actor) or output/kernel|bias (critic) [nh][nout], [nout]
struct NetLayout {
    int nin, nh, nl, nout, ln;
    long w[MAXL], b[MAXL], beta[MAXL], gamma[MAXL], wo, bo, P;
};

__host__ __device__ inline NetLayout make_layout(int nin, int nh, int nl, int nout, int ln) {
    NetLayout L{};
    L.nin = nin; L.nh = nh; L.nl = nl; L.nout = nout; L.ln = ln;
    long o = 0;
    int k = nin;
    for (int i = 0; i < nl; ++i) {
        L.w[i] = o; o += (long)k * nh;
        L.b[i] = o; o += nh;
        if (ln) { L.beta[i] = o; o += nh; L.gamma[i] = o; o += nh; } else { L.beta[i] = L.gamma[i] = -1; }
        k = nh;
    }
    L.wo = o; o += (long)nh * nout;
    L.bo = o; o += nout;
    L.P = o;
    return L;
}

struct Acts {                 // forward activations of one MLP evaluation, kept for its backward pass
    float* h[MAXL];           // [B][nh] post-activation
    float* xh[MAXL];          // [B][nh] normalised pre-activation (layer_norm)
    float* is[MAXL];          // [B] 1/sqrt(var + eps) (layer_norm)
};

struct Carver {
    char* base; size_t off;
    __host__ __device__ float* f(size_t n) {
        float* p = base ? (float*)(base + off) : nullptr;
        off += (n * sizeof(float) + 255) / 256 * 256;
        return p;
    }
};

Acts carve_acts(Carver& c, int B, int nh, int nl, int ln) {
    Acts a{};
    for (int l = 0; l < nl; ++l) {
        a.h[l] = c.f((size_t)B * nh);
        if (ln) { a.xh[l] = c.f((size_t)B * nh); a.is[l] = c.f(B); }
    }
    return a;
}

// ---- block-wide building blocks (any blockDim.x that is a multiple of 64) ---------------------------------------

__device__ __forceinline__ float act_f(float u, int act) {
    return act == MRL_ACT_TANH ? tanhf(u) : (act == MRL_ACT_RELU ? fmaxf(u, 0.f) : u);
}
// d act / d u expressed through the output y (TF's TanhGrad dy * (1 - y*y), ReluGrad dy * (y > 0))
__device__ __forceinline__ float act_bwd(float dy, float y, int act) {
    return act == MRL_ACT_TANH ? dy * (1.f - y * y) : (act == MRL_ACT_RELU ? (y > 0.f ? dy : 0.f) : dy);
}

// Compensated fp32 accumulation (Ogita, Rump and Oishi's Dot2 / Sum2): each product's rounding error comes from an FMA, each
// addition's from TwoSum, and the errors are summed in a second fp32 word.  The result is as if the sum had been accumulated in
// twice the working precision and rounded once, so a batch or feature sum adds no error beyond the rounding of its inputs.
// Storage and arithmetic stay fp32 (the file is built with -ffp-contract=off, which keeps TwoSum intact).
struct Acc2 {
    float s = 0.f, c = 0.f;
    __device__ __forceinline__ void add(float x) {
        const float t = s + x, z = t - s;
        c += (s - (t - z)) + (x - z);
        s = t;
    }
    __device__ __forceinline__ void fma(float a, float b) {
        const float p = a * b;
        c += fmaf(a, b, -p);
        add(p);
    }
    __device__ __forceinline__ float get() const { return s + c; }
};

// deterministic block sum; every thread gets the result.  sh: >= 16 floats of LDS
__device__ float block_sum(float v, float* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) r += sh[i];
    return r;
}

// Y[b][n] = act(sum_k X[b][k] W[k][n] + bias[n]) (tf.layers.dense / fc: matmul, then bias add).  Four rows per thread so that
// each weight load feeds four FMAs.
__device__ void dense_fwd(const float* __restrict__ X, int ldx, int K, int B, const float* __restrict__ W,
                          const float* __restrict__ bias, int N, float* __restrict__ Y, int ldy, int act) {
    const int nq = (B + 3) >> 2;
    for (int i = threadIdx.x; i < nq * N; i += blockDim.x) {
        const int q = i / N, n = i - q * N, b0 = q * 4;
        const float* x0 = X + (long)b0 * ldx;
        const float* x1 = X + (long)min(b0 + 1, B - 1) * ldx;
        const float* x2 = X + (long)min(b0 + 2, B - 1) * ldx;
        const float* x3 = X + (long)min(b0 + 3, B - 1) * ldx;
        Acc2 a0, a1, a2, a3;
        for (int k = 0; k < K; ++k) {
            const float w = W[(long)k * N + n];
            a0.fma(x0[k], w); a1.fma(x1[k], w); a2.fma(x2[k], w); a3.fma(x3[k], w);
        }
        const float bb = bias[n];
        Y[(long)b0 * ldy + n] = act_f(a0.get() + bb, act);
        if (b0 + 1 < B) Y[(long)(b0 + 1) * ldy + n] = act_f(a1.get() + bb, act);
        if (b0 + 2 < B) Y[(long)(b0 + 2) * ldy + n] = act_f(a2.get() + bb, act);
        if (b0 + 3 < B) Y[(long)(b0 + 3) * ldy + n] = act_f(a3.get() + bb, act);
    }
}

// layer_norm (moments over the row, biased variance) + activation, in place on Y [B][N] (common/models.py:97-99)
__device__ void ln_act(float* __restrict__ Y, float* __restrict__ XH, float* __restrict__ IS, const float* __restrict__ beta,
                       const float* __restrict__ gamma, int B, int N, int act, float* __restrict__ rs) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* z = Y + (long)b * N;
        Acc2 s;
        for (int c = 0; c < N; ++c) s.add(z[c]);
        const float mean = s.get() / (float)N;
        Acc2 q;
        for (int c = 0; c < N; ++c) { const float d = z[c] - mean; q.fma(d, d); }
        rs[b] = mean;
        IS[b] = 1.f / sqrtf(q.get() / (float)N + LN_EPS);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B * N; i += blockDim.x) {
        const int b = i / N, c = i - b * N;
        const float xh = (Y[i] - rs[b]) * IS[b];
        XH[i] = xh;
        Y[i] = act_f(xh * gamma[c] + beta[c], act);
    }
}

// D [B][N]: gradient w.r.t. the layer's output H in, gradient w.r.t. its pre-norm linear output out (in place).
// dbeta / dgamma (may be null) receive the layer-norm parameter gradients.
__device__ void act_ln_bwd(float* __restrict__ D, const float* __restrict__ H, const float* __restrict__ XH,
                           const float* __restrict__ IS, const float* __restrict__ gamma, int B, int N, int act, int ln,
                           float* __restrict__ dbeta, float* __restrict__ dgamma, float* __restrict__ rs) {
    for (int i = threadIdx.x; i < B * N; i += blockDim.x) D[i] = act_bwd(D[i], H[i], act);
    if (!ln) return;
    __syncthreads();
    const int ncol = dbeta ? N : 0;
    for (int i = threadIdx.x; i < ncol + B; i += blockDim.x) {
        if (i < ncol) {
            Acc2 sb, sg;
            for (int b = 0; b < B; ++b) { const float d = D[(long)b * N + i]; sb.add(d); sg.fma(d, XH[(long)b * N + i]); }
            dbeta[i] = sb.get();
            dgamma[i] = sg.get();
        } else {
            const int b = i - ncol;
            const float* d = D + (long)b * N;
            const float* x = XH + (long)b * N;
            Acc2 m1, m2;
            for (int c = 0; c < N; ++c) { const float g = d[c] * gamma[c]; m1.add(g); m2.fma(g, x[c]); }
            rs[2 * b] = m1.get() / (float)N;
            rs[2 * b + 1] = m2.get() / (float)N;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B * N; i += blockDim.x) {
        const int b = i / N, c = i - b * N;
        D[i] = IS[b] * ((D[i] * gamma[c] - rs[2 * b]) - XH[i] * rs[2 * b + 1]);
    }
}

// backward of Y = X W + b given dZ [B][N]: dW [K][N] = X^T dZ, db [N] = column sums (both may be null), dX[b][k] for
// k in [k0, K) (dX may be null) written at dX + b*lddx + k.  One pass over all three kinds of output.
__device__ void dense_bwd(const float* __restrict__ X, int ldx, int K, int B, const float* __restrict__ W, int N,
                          const float* __restrict__ dZ, float* __restrict__ dW, float* __restrict__ db,
                          float* __restrict__ dX, int lddx, int k0) {
    const int nW = dW ? K * N : 0, nB = db ? N : 0, kx = K - k0, nX = dX ? B * kx : 0;
    for (int i = threadIdx.x; i < nW + nB + nX; i += blockDim.x) {
        if (i < nW) {
            const int k = i / N, n = i - k * N;
            Acc2 s;
            for (int b = 0; b < B; ++b) s.fma(X[(long)b * ldx + k], dZ[(long)b * N + n]);
            dW[i] = s.get();
        } else if (i < nW + nB) {
            const int n = i - nW;
            Acc2 s;
            for (int b = 0; b < B; ++b) s.add(dZ[(long)b * N + n]);
            db[n] = s.get();
        } else {
            const int j = i - nW - nB, b = j / kx, k = k0 + (j - b * kx);
            const float* w = W + (long)k * N;
            const float* d = dZ + (long)b * N;
            Acc2 s;
            for (int n = 0; n < N; ++n) s.fma(d[n], w[n]);
            dX[(long)b * lddx + k] = s.get();
        }
    }
}

// whole MLP forward: body (fc -> [layer_norm] -> act) x nl, then the final dense layer with out_act into out [B][ldo]
__device__ void mlp_fwd(const float* P, const NetLayout& L, const float* X, int ldx, int B, const Acts& a, int act,
                        float* out, int ldo, int out_act, float* rs) {
    const float* in = X;
    int ldin = ldx, K = L.nin;
    for (int l = 0; l < L.nl; ++l) {
        dense_fwd(in, ldin, K, B, P + L.w[l], P + L.b[l], L.nh, a.h[l], L.nh, L.ln ? MRL_ACT_NONE : act);
        __syncthreads();
        if (L.ln) {
            ln_act(a.h[l], a.xh[l], a.is[l], P + L.beta[l], P + L.gamma[l], B, L.nh, act, rs);
            __syncthreads();
        }
        in = a.h[l]; ldin = L.nh; K = L.nh;
    }
    dense_fwd(in, ldin, K, B, P + L.wo, P + L.bo, L.nout, out, ldo, out_act);
    __syncthreads();
}

// whole MLP backward from dOut [B][nout] (gradient w.r.t. the final dense layer's linear output).  G (may be null): weight
// gradients in the flat layout.  dX (may be null): gradient w.r.t. input columns [k0, nin).  d0/d1: [B][nh] scratch.
__device__ void mlp_bwd(const float* P, const NetLayout& L, const float* X, int ldx, int B, const Acts& a, int act,
                        const float* dOut, float* G, float* dX, int lddx, int k0, float* d0, float* d1, float* rs) {
    const int H = L.nh;
    dense_bwd(a.h[L.nl - 1], H, H, B, P + L.wo, L.nout, dOut, G ? G + L.wo : nullptr, G ? G + L.bo : nullptr, d0, H, 0);
    __syncthreads();
    float* cur = d0;
    float* nxt = d1;
    for (int l = L.nl - 1; l >= 0; --l) {
        act_ln_bwd(cur, a.h[l], a.xh[l], a.is[l], L.ln ? P + L.gamma[l] : nullptr, B, H, act, L.ln,
                   (G && L.ln) ? G + L.beta[l] : nullptr, (G && L.ln) ? G + L.gamma[l] : nullptr, rs);
        __syncthreads();
        const float* in = l ? a.h[l - 1] : X;
        float* dn = l ? nxt : dX;
        dense_bwd(in, l ? H : ldx, l ? H : L.nin, B, P + L.w[l], H, cur, G ? G + L.w[l] : nullptr, G ? G + L.b[l] : nullptr,
                  dn, l ? H : lddx, l ? 0 : k0);
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
    }
}

// obs_rms statistics as the reference's graph computes them (common/mpi_running_mean_std.py:29-30): f64 sums, cast to f32,
// std = sqrt(max(f32(sumsq/count) - mean^2, 1e-2)); then ddpg_learner.py:17-20 normalize and :104-107 clip to [-5, 5]
__device__ __forceinline__ float norm_obs(float x, const double* rms, int D, int d, int on) {
    float y = x;
    if (on) {
        const double cnt = rms[2 * D];
        const float mean = (float)(rms[d] / cnt);
        const float std = sqrtf(fmaxf((float)(rms[D + d] / cnt) - mean * mean, 1e-2f));
        y = (x - mean) / (std + 1e-8f);
    }
    return fminf(fmaxf(y, -5.f), 5.f);
}
__device__ __forceinline__ void rms_scalar(const double* r, float& mean, float& std) {
    mean = (float)(r[0] / r[2]);
    std = sqrtf(fmaxf((float)(r[1] / r[2]) - mean * mean, 1e-2f));
}

struct TrainArgs {
    mrl_ddpg_state s;
    NetLayout la, lc;
    int D, A, B, act, norm_obs, norm_ret, popart, soft, has_clip;
    float gamma, one_minus_tau, tau, l2, clip;
    const int64_t* idx;
    const float* hp;          // device f32 [2]: -a of the actor's and the critic's MpiAdam step
    float* losses;            // [2]: critic_loss, actor_loss
    float* grads_out;         // [Pa + Pc] or null
    // workspace
    float *X0c, *X0q, *X1c, *q1, *qc, *qa, *tn, *rew, *term, *d0, *d1, *dX, *dzo, *rs, *ga, *gc;
    Acts ta, tc, ca, aa, qq;
};

// per-tensor tf.clip_by_norm (tf_util.py:flatgrad): g <- g * c / max(||g||, c)
__device__ void clip_tensor(float* g, long n, float c, float* sh) {
    Acc2 s;
    for (long i = threadIdx.x; i < n; i += blockDim.x) s.fma(g[i], g[i]);
    const float l2sum = block_sum(s.get(), sh);
    const float l2norm = l2sum > 0.f ? sqrtf(l2sum) : l2sum;
    const float den = fmaxf(l2norm, c);
    for (long i = threadIdx.x; i < n; i += blockDim.x) g[i] = (g[i] * c) / den;
}
__device__ void clip_net(float* G, const NetLayout& L, float c, float* sh) {
    int k = L.nin;
    for (int l = 0; l < L.nl; ++l) {
        clip_tensor(G + L.w[l], (long)k * L.nh, c, sh);
        clip_tensor(G + L.b[l], L.nh, c, sh);
        if (L.ln) { clip_tensor(G + L.beta[l], L.nh, c, sh); clip_tensor(G + L.gamma[l], L.nh, c, sh); }
        k = L.nh;
    }
    clip_tensor(G + L.wo, (long)L.nh * L.nout, c, sh);
    clip_tensor(G + L.bo, L.nout, c, sh);
}

// MpiAdam.update, common/mpi_adam.py:38-41 (f32 m, v; a = lr*sqrt(1-beta2^t)/(1-beta1^t) in f64 on the host, negated and
// rounded to f32 as NumPy does in `(- a) * self.m`)
__device__ void mpi_adam(float* p, const float* g, float* m, float* v, long P, float na) {
    for (long i = threadIdx.x; i < P; i += blockDim.x) {
        const float gi = g[i];
        const float mi = 0.9f * m[i] + 0.1f * gi;
        const float vi = 0.999f * v[i] + 0.001f * (gi * gi);
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] + (na * mi) / (sqrtf(vi) + 1e-8f);
    }
}

__global__ __launch_bounds__(TRAIN_THREADS) void ddpg_train_kernel(TrainArgs a) {
    __shared__ float sh[16];
    __shared__ float sret[4];
    const mrl_ddpg_state& s = a.s;
    const int D = a.D, A = a.A, B = a.B, W = D + A, H = a.la.nh;
    const long start = s.ring_pos[0], limit = s.limit;

    // 1+2. gather the batch at (start + idx) % limit (memory.py:19-20) and normalise / clip obs0, obs1 (ddpg_learner.py:104-107)
    for (int i = threadIdx.x; i < B * W; i += blockDim.x) {
        const int b = i / W, c = i - b * W;
        const long r = (start + a.idx[b]) % limit;
        if (c < D) {
            const float x0 = norm_obs(s.obs0[r * D + c], s.obs_rms, D, c, a.norm_obs);
            a.X0c[i] = x0;
            a.X0q[i] = x0;
            a.X1c[i] = norm_obs(s.obs1[r * D + c], s.obs_rms, D, c, a.norm_obs);
        } else {
            a.X0c[i] = s.actions[r * A + (c - D)];
        }
        if (c == 0) { a.rew[b] = s.rewards[r]; a.term[b] = s.terminals1[r]; }
    }
    __syncthreads();

    // 3. target_Q = r + (1 - d) * gamma * denorm(Q'(obs1, mu'(obs1)))   (ddpg_learner.py:134-135)
    mlp_fwd(s.target_actor, a.la, a.X1c, W, B, a.ta, a.act, a.X1c + D, W, MRL_ACT_TANH, a.rs);
    mlp_fwd(s.target_critic, a.lc, a.X1c, W, B, a.tc, a.act, a.q1, 1, MRL_ACT_NONE, a.rs);
    float rm = 0.f, rsd = 1.f;
    if (a.norm_ret) rms_scalar(s.ret_rms, rm, rsd);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float q = a.norm_ret ? a.q1[b] * rsd + rm : a.q1[b];
        a.q1[b] = a.rew[b] + ((1.f - a.term[b]) * a.gamma) * q;          // target_Q, kept in q1
    }
    __syncthreads();

    // 4. pop-art (ddpg_learner.py:217-236, 308-317): ret_rms.update(target_Q) in f64, then renormalise the output layers of
    //    the critic AND the target critic with the old and new statistics
    if (a.norm_ret && a.popart) {
        if (threadIdx.x == 0) {
            double sm = 0.0, sq = 0.0;
            for (int b = 0; b < B; ++b) { const double x = (double)a.q1[b]; sm += x; sq += x * x; }
            double* r = s.ret_rms;
            r[0] += sm; r[1] += sq; r[2] += (double)B;
            float nm, ns;
            rms_scalar(r, nm, ns);
            sret[0] = nm; sret[1] = ns;
        }
        __syncthreads();
        const float nm = sret[0], ns = sret[1];
        for (int i = threadIdx.x; i < 2 * (H + 1); i += blockDim.x) {
            float* net = i < H + 1 ? s.critic : s.target_critic;
            const int j = i < H + 1 ? i : i - (H + 1);
            if (j < H) { float* M = net + a.lc.wo + j; *M = (*M * rsd) / ns; }
            else { float* bb = net + a.lc.bo; *bb = ((*bb * rsd + rm) - nm) / ns; }
        }
        __syncthreads();
        rm = nm; rsd = ns;
    }

    // 5. critic loss on the normalised target (ddpg_learner.py:198-213) and its gradient
    mlp_fwd(s.critic, a.lc, a.X0c, W, B, a.ca, a.act, a.qc, 1, MRL_ACT_NONE, a.rs);
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float t = a.norm_ret ? (a.q1[b] - rm) / (rsd + 1e-8f) : a.q1[b];
        const float e = a.qc[b] - t;
        part = fmaf(e, e, part);
        a.tn[b] = (2.f * e) / (float)B;                                 // d loss / d Q
    }
    const float mse = block_sum(part, sh) / (float)B;
    mlp_bwd(s.critic, a.lc, a.X0c, W, B, a.ca, a.act, a.tn, a.gc, nullptr, 0, 0, a.d0, a.d1, a.rs);
    float reg = 0.f;
    if (a.l2 > 0.f) {          // l2 over critic mlp_fc*/w only, output and LayerNorm excluded (ddpg_learner.py:201-210)
        int k = a.lc.nin;
        for (int l = 0; l < a.lc.nl; ++l) {
            const long n = (long)k * H;
            const float* w = s.critic + a.lc.w[l];
            float* g = a.gc + a.lc.w[l];
            Acc2 ss;
            for (long i = threadIdx.x; i < n; i += blockDim.x) { ss.fma(w[i], w[i]); g[i] = g[i] + a.l2 * w[i]; }
            reg += a.l2 * (block_sum(ss.get(), sh) / 2.f);
            k = H;
        }
    }

    // 6. actor loss -mean(denorm(Q(obs0, mu(obs0)))) through the critic from before this step's update (ddpg_learner.py:186)
    mlp_fwd(s.actor, a.la, a.X0q, W, B, a.aa, a.act, a.X0q + D, W, MRL_ACT_TANH, a.rs);
    mlp_fwd(s.critic, a.lc, a.X0q, W, B, a.qq, a.act, a.qa, 1, MRL_ACT_NONE, a.rs);
    float qp = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        qp += a.norm_ret ? a.qa[b] * rsd + rm : a.qa[b];
        a.tn[b] = a.norm_ret ? -rsd / (float)B : -1.f / (float)B;
    }
    const float actor_loss = -(block_sum(qp, sh) / (float)B);
    mlp_bwd(s.critic, a.lc, a.X0q, W, B, a.qq, a.act, a.tn, nullptr, a.dX, W, D, a.d0, a.d1, a.rs);
    for (int i = threadIdx.x; i < B * A; i += blockDim.x) {
        const int b = i / A, j = i - b * A;
        a.dzo[i] = act_bwd(a.dX[(long)b * W + D + j], a.X0q[(long)b * W + D + j], MRL_ACT_TANH);
    }
    __syncthreads();
    mlp_bwd(s.actor, a.la, a.X0q, W, B, a.aa, a.act, a.dzo, a.ga, nullptr, 0, 0, a.d0, a.d1, a.rs);

    // 7. per-variable clip_by_norm (tf_util.py:flatgrad)
    if (a.has_clip) {
        clip_net(a.ga, a.la, a.clip, sh);
        clip_net(a.gc, a.lc, a.clip, sh);
        __syncthreads();
    }
    if (a.grads_out) {
        for (long i = threadIdx.x; i < a.la.P; i += blockDim.x) a.grads_out[i] = a.ga[i];
        for (long i = threadIdx.x; i < a.lc.P; i += blockDim.x) a.grads_out[a.la.P + i] = a.gc[i];
    }
    // 8. MpiAdam per network, both after both gradients (ddpg_learner.py:270-271)
    const float na = a.hp[0], nc = a.hp[1];
    mpi_adam(s.actor, a.ga, s.actor_m, s.actor_v, a.la.P, na);
    mpi_adam(s.critic, a.gc, s.critic_m, s.critic_v, a.lc.P, nc);
    // soft target update (ddpg_learner.py:36-47, update_target_net), fused behind a flag
    if (a.soft) {
        __syncthreads();
        for (long i = threadIdx.x; i < a.la.P; i += blockDim.x)
            s.target_actor[i] = a.one_minus_tau * s.target_actor[i] + a.tau * s.actor[i];
        for (long i = threadIdx.x; i < a.lc.P; i += blockDim.x)
            s.target_critic[i] = a.one_minus_tau * s.target_critic[i] + a.tau * s.critic[i];
    }
    // 9. losses (train() returns critic_loss, actor_loss)
    if (threadIdx.x == 0) { a.losses[0] = mse + reg; a.losses[1] = actor_loss; }
}

// ---- act side ------------------------------------------------------------------------------------------------------
struct ActArgs {
    NetLayout la, lc;
    int D, A, n, act, norm_obs, norm_ret;
    const float *actor, *pactor, *critic, *obs, *actions_in;
    const double *obs_rms, *ret_rms, *noise;
    float *actions_out, *q_out;
    char* ws; size_t slice;
    int ln;
};

struct ActWs { float *X, *atmp, *q, *rs; Acts s; };
__host__ __device__ inline size_t act_carve(char* base, const NetLayout& la, int D, int A, int R, ActWs* w) {
    Carver c{base, 0};
    ActWs t;
    t.X = c.f((size_t)R * (D + A));
    t.atmp = c.f((size_t)R * A);
    t.q = c.f(R);
    t.rs = c.f(2 * R);
    for (int l = 0; l < la.nl; ++l) {
        t.s.h[l] = c.f((size_t)R * la.nh);
        if (la.ln) { t.s.xh[l] = c.f((size_t)R * la.nh); t.s.is[l] = c.f(R); } else { t.s.xh[l] = t.s.is[l] = nullptr; }
    }
    if (w) *w = t;
    return c.off;
}

// ddpg_learner.py:step (239-257): action from the actor (the perturbed actor when param noise is on), Q from the critic on
// (obs, UNPERTURBED actor(obs)) -- critic_with_actor_tf -- or on (obs, actions_in) when given (critic_tf, get_stats);
// action += noise (one f64 vector for every row, as `action += noise` broadcasts), clip to [-1, 1]
__global__ __launch_bounds__(ACT_THREADS) void ddpg_act_kernel(ActArgs a) {
    const int r0 = blockIdx.x * ACT_ROWS, R = min(ACT_ROWS, a.n - r0);
    const int D = a.D, A = a.A, W = D + A;
    ActWs w;
    act_carve(a.ws + (size_t)blockIdx.x * a.slice, a.la, D, A, ACT_ROWS, &w);
    for (int i = threadIdx.x; i < R * W; i += blockDim.x) {
        const int b = i / W, c = i - b * W;
        const long r = r0 + b;
        w.X[i] = c < D ? norm_obs(a.obs[r * D + c], a.obs_rms, D, c, a.norm_obs)
                       : (a.actions_in ? a.actions_in[r * A + (c - D)] : 0.f);
    }
    __syncthreads();
    if (a.pactor) mlp_fwd(a.pactor, a.la, w.X, W, R, w.s, a.act, w.atmp, A, MRL_ACT_TANH, w.rs);
    // actor output goes into the critic's action columns unless the critic is to see actions_in
    float* aout = a.actions_in ? w.atmp : w.X + D;
    const int ldo = a.actions_in ? A : W;
    if (!a.pactor || !a.actions_in) mlp_fwd(a.actor, a.la, w.X, W, R, w.s, a.act, aout, ldo, MRL_ACT_TANH, w.rs);
    if (a.q_out) {
        mlp_fwd(a.critic, a.lc, w.X, W, R, w.s, a.act, w.q, 1, MRL_ACT_NONE, w.rs);
        float rm = 0.f, rsd = 1.f;
        if (a.norm_ret) rms_scalar(a.ret_rms, rm, rsd);
        for (int b = threadIdx.x; b < R; b += blockDim.x) a.q_out[r0 + b] = a.norm_ret ? w.q[b] * rsd + rm : w.q[b];
    }
    if (a.actions_out) {
        for (int i = threadIdx.x; i < R * A; i += blockDim.x) {
            const int b = i / A, j = i - b * A;
            float x = a.pactor ? w.atmp[i] : (a.actions_in ? w.atmp[i] : w.X[(long)b * W + D + j]);
            if (a.noise) x = (float)((double)x + a.noise[j]);
            a.actions_out[(long)(r0 + b) * A + j] = fminf(fmaxf(x, -1.f), 1.f);
        }
    }
}

// ---- adaptive_policy_distance (ddpg_learner.py:168-173): sqrt(mean((mu(obs) - mu~(obs))^2)) on a batch of the ring --------
__global__ __launch_bounds__(TRAIN_THREADS) void ddpg_distance_kernel(mrl_ddpg_state s, NetLayout la, int D, int A, int B,
                                                                      int act, int nobs, const float* pactor,
                                                                      const int64_t* idx, float* out, float* X, float* a0,
                                                                      float* a1, float* rs, Acts st) {
    __shared__ float sh[16];
    const long start = s.ring_pos[0];
    for (int i = threadIdx.x; i < B * D; i += blockDim.x) {
        const int b = i / D, c = i - b * D;
        const long r = (start + idx[b]) % s.limit;
        X[i] = norm_obs(s.obs0[r * D + c], s.obs_rms, D, c, nobs);
    }
    __syncthreads();
    mlp_fwd(s.actor, la, X, D, B, st, act, a0, A, MRL_ACT_TANH, rs);
    mlp_fwd(pactor, la, X, D, B, st, act, a1, A, MRL_ACT_TANH, rs);
    Acc2 p;
    for (int i = threadIdx.x; i < B * A; i += blockDim.x) { const float d = a0[i] - a1[i]; p.fma(d, d); }
    const float m = block_sum(p.get(), sh) / (float)(B * A);
    if (threadIdx.x == 0) *out = sqrtf(m);
}

// ---- get_perturbed_actor_updates (ddpg_learner.py:50-62): perturbable (non-LayerNorm) tensors get var + stddev * noise ---
__global__ __launch_bounds__(256) void ddpg_perturb_kernel(const float* __restrict__ actor, float* __restrict__ out,
                                                           const float* __restrict__ noise, float stddev, NetLayout L) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < L.P; i += (long)gridDim.x * 256L) {
        bool lnv = false;
        for (int l = 0; l < L.nl; ++l) lnv |= L.ln && i >= L.beta[l] && i < L.gamma[l] + L.nh;
        // tf.random_normal(mean=0, stddev=s) = n * s + 0
        out[i] = lnv ? actor[i] : actor[i] + (noise[i] * stddev + 0.f);
    }
}

// soft target update as its own launch: target <- (1 - tau) * target + tau * var   (ddpg_learner.py:36-47)
__global__ __launch_bounds__(256) void ddpg_soft_kernel(float* __restrict__ t, const float* __restrict__ v, long P, float omt,
                                                        float tau) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < P; i += (long)gridDim.x * 256L) t[i] = omt * t[i] + tau * v[i];
}

// ---- store_transition (ddpg_learner.py:259-266, memory.py:24-35,71-79) --------------------------------------------------
__global__ __launch_bounds__(512) void ddpg_store_kernel(mrl_ddpg_state s, int D, int A, int n, const float* __restrict__ obs0,
                                                         const float* __restrict__ action, const float* __restrict__ reward,
                                                         const float* __restrict__ obs1, const uint8_t* __restrict__ term,
                                                         float reward_scale, int update_rms) {
    const long start0 = s.ring_pos[0], len0 = s.ring_pos[1], limit = s.limit;
    // append number b lands at (start + length - 1) % limit after its own update = (start0 + len0 + b) % limit; when more
    // rows than the ring holds arrive at once only the last `limit` of them survive
    const int first = n > limit ? (int)(n - limit) : 0;
    const int W = 2 * D + A + 2;
    for (long i = threadIdx.x; i < (long)(n - first) * W; i += blockDim.x) {
        const int b = first + (int)(i / W), c = (int)(i % W);
        const long slot = (start0 + len0 + b) % limit;
        if (c < D) s.obs0[slot * D + c] = obs0[(long)b * D + c];
        else if (c < 2 * D) s.obs1[slot * D + c - D] = obs1[(long)b * D + c - D];
        else if (c < 2 * D + A) s.actions[slot * A + c - 2 * D] = action[(long)b * A + c - 2 * D];
        else if (c == 2 * D + A) s.rewards[slot] = reward[b] * reward_scale;
        else s.terminals1[slot] = term[b] ? 1.f : 0.f;
    }
    // obs_rms.update(np.array([obs0[b]])) row by row: f64 sums in row order, count += 1 per row
    if (update_rms) {
        for (int d = threadIdx.x; d <= D; d += blockDim.x) {
            if (d < D) {
                double sm = s.obs_rms[d], sq = s.obs_rms[D + d];
                for (int b = 0; b < n; ++b) { const double x = (double)obs0[(long)b * D + d]; sm += x; sq += x * x; }
                s.obs_rms[d] = sm;
                s.obs_rms[D + d] = sq;
            } else {
                double c = s.obs_rms[2 * D];
                for (int b = 0; b < n; ++b) c += 1.0;
                s.obs_rms[2 * D] = c;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long tot = len0 + n;
        s.ring_pos[1] = tot < limit ? tot : limit;
        s.ring_pos[0] = (start0 + (tot > limit ? tot - limit : 0)) % limit;
    }
}

int check_desc(const mrl_ddpg_desc* d) {
    if (!d) return MRL_EINVAL;
    if (d->num_layers < 1 || d->num_layers > MAXL) return MRL_EUNSUP;
    if (d->num_hidden < 32 || d->num_hidden > 256 || d->num_hidden % 32) return MRL_EUNSUP;
    if (d->activation != MRL_ACT_TANH && d->activation != MRL_ACT_RELU) return MRL_EUNSUP;
    if (d->ob_dim < 1 || d->ob_dim > 4096) return MRL_EUNSUP;
    if (d->nact < 1 || d->nact > 32) return MRL_EUNSUP;
    return 0;
}
NetLayout actor_layout(const mrl_ddpg_desc* d) {
    return make_layout(d->ob_dim, d->num_hidden, d->num_layers, d->nact, d->layer_norm ? 1 : 0);
}
NetLayout critic_layout(const mrl_ddpg_desc* d) {
    return make_layout(d->ob_dim + d->nact, d->num_hidden, d->num_layers, 1, d->layer_norm ? 1 : 0);
}

size_t train_carve(const mrl_ddpg_desc* d, int B, char* base, TrainArgs* a) {
    Carver c{base, 0};
    const int D = d->ob_dim, A = d->nact, W = D + A, H = d->num_hidden, L = d->num_layers, ln = d->layer_norm ? 1 : 0;
    TrainArgs t{};
    t.X0c = c.f((size_t)B * W); t.X0q = c.f((size_t)B * W); t.X1c = c.f((size_t)B * W); t.dX = c.f((size_t)B * W);
    t.q1 = c.f(B); t.qc = c.f(B); t.qa = c.f(B); t.tn = c.f(B); t.rew = c.f(B); t.term = c.f(B);
    t.d0 = c.f((size_t)B * H); t.d1 = c.f((size_t)B * H); t.dzo = c.f((size_t)B * A); t.rs = c.f(2 * (size_t)B);
    t.ga = c.f(actor_layout(d).P); t.gc = c.f(critic_layout(d).P);
    t.ta = carve_acts(c, B, H, L, ln); t.tc = carve_acts(c, B, H, L, ln); t.ca = carve_acts(c, B, H, L, ln);
    t.aa = carve_acts(c, B, H, L, ln); t.qq = carve_acts(c, B, H, L, ln);
    if (a) {
        t.s = a->s; t.la = a->la; t.lc = a->lc; t.D = a->D; t.A = a->A; t.B = a->B; t.act = a->act;
        t.norm_obs = a->norm_obs; t.norm_ret = a->norm_ret; t.popart = a->popart; t.soft = a->soft; t.has_clip = a->has_clip;
        t.gamma = a->gamma; t.one_minus_tau = a->one_minus_tau; t.tau = a->tau; t.l2 = a->l2; t.clip = a->clip;
        t.idx = a->idx; t.hp = a->hp; t.losses = a->losses; t.grads_out = a->grads_out;
        *a = t;
    }
    return c.off;
}

bool state_ok(const mrl_ddpg_state* s, bool ring) {
    if (!s || !s->actor || !s->critic || !s->obs_rms) return false;
    if (ring && (!s->obs0 || !s->obs1 || !s->actions || !s->rewards || !s->terminals1 || !s->ring_pos || s->limit < 1)) return false;
    return true;
}

}  // namespace

extern "C" long mrl_ddpg_num_params(const mrl_ddpg_desc* d, int net) {
    if (check_desc(d)) return -1;
    return net == 0 ? actor_layout(d).P : critic_layout(d).P;
}

extern "C" size_t mrl_ddpg_workspace_bytes(const mrl_ddpg_desc* d, int B) {
    if (check_desc(d) || B < 1) return 0;
    const size_t tr = train_carve(d, B, nullptr, nullptr);
    const NetLayout la = actor_layout(d);
    const size_t act = act_carve(nullptr, la, d->ob_dim, d->nact, ACT_ROWS, nullptr) * (size_t)((B + ACT_ROWS - 1) / ACT_ROWS);
    return tr > act ? tr : act;
}

extern "C" int mrl_ddpg_train_step(const mrl_ddpg_desc* d, const mrl_ddpg_state* s, const int64_t* idx, int B,
                                   const float* neg_alpha, float gamma, double tau, float critic_l2_reg, float clip_norm,
                                   int soft_update, float* grads_out, float* losses_out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (B < 1 || B > 1024) return MRL_EUNSUP;
    if (!state_ok(s, true) || !s->target_actor || !s->target_critic || !s->actor_m || !s->actor_v || !s->critic_m ||
        !s->critic_v || !idx || !neg_alpha || !losses_out || !workspace)
        return MRL_EINVAL;
    if (d->normalize_returns && !s->ret_rms) return MRL_EINVAL;
    if (workspace_bytes < train_carve(d, B, nullptr, nullptr)) return MRL_ENOSPC;
    TrainArgs a{};
    a.s = *s; a.la = actor_layout(d); a.lc = critic_layout(d);
    a.D = d->ob_dim; a.A = d->nact; a.B = B; a.act = d->activation;
    a.norm_obs = d->normalize_observations ? 1 : 0; a.norm_ret = d->normalize_returns ? 1 : 0;
    a.popart = d->popart ? 1 : 0; a.soft = soft_update ? 1 : 0;
    a.has_clip = clip_norm > 0.f; a.clip = clip_norm;
    a.gamma = gamma; a.tau = (float)tau; a.one_minus_tau = (float)(1.0 - tau); a.l2 = critic_l2_reg;
    a.idx = idx; a.hp = neg_alpha; a.losses = losses_out; a.grads_out = grads_out;
    train_carve(d, B, (char*)workspace, &a);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("ddpg.train_step", -1.0, -1.0, st);
    hipLaunchKernelGGL(ddpg_train_kernel, dim3(1), dim3(TRAIN_THREADS), 0, st, a);
    MRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrl_ddpg_soft_update(const mrl_ddpg_desc* d, const mrl_ddpg_state* s, double tau, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!s || !s->actor || !s->critic || !s->target_actor || !s->target_critic) return MRL_EINVAL;
    const float omt = (float)(1.0 - tau), tf = (float)tau;
    hipStream_t st = (hipStream_t)stream;
    const long Pa = actor_layout(d).P, Pc = critic_layout(d).P;
    hipLaunchKernelGGL(ddpg_soft_kernel, dim3((unsigned)std::min<long>((Pa + 255) / 256, 1024)), dim3(256), 0, st, s->target_actor,
                       (const float*)s->actor, Pa, omt, tf);
    MRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ddpg_soft_kernel, dim3((unsigned)std::min<long>((Pc + 255) / 256, 1024)), dim3(256), 0, st, s->target_critic,
                       (const float*)s->critic, Pc, omt, tf);
    MRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrl_ddpg_act(const mrl_ddpg_desc* d, const mrl_ddpg_state* s, const float* perturbed_actor, const float* obs,
                            const float* actions_in, const double* noise, int n, float* actions_out, float* q_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (n < 1) return MRL_EINVAL;
    if (!state_ok(s, false) || !obs || !workspace || (!actions_out && !q_out)) return MRL_EINVAL;
    if (d->normalize_returns && !s->ret_rms) return MRL_EINVAL;
    ActArgs a{};
    a.la = actor_layout(d); a.lc = critic_layout(d);
    a.D = d->ob_dim; a.A = d->nact; a.n = n; a.act = d->activation;
    a.norm_obs = d->normalize_observations ? 1 : 0; a.norm_ret = d->normalize_returns ? 1 : 0;
    a.actor = s->actor; a.pactor = perturbed_actor; a.critic = s->critic; a.obs = obs; a.actions_in = actions_in;
    a.obs_rms = s->obs_rms; a.ret_rms = s->ret_rms; a.noise = noise;
    a.actions_out = actions_out; a.q_out = q_out;
    a.slice = act_carve(nullptr, a.la, a.D, a.A, ACT_ROWS, nullptr);
    const int nb = (n + ACT_ROWS - 1) / ACT_ROWS;
    if (workspace_bytes < a.slice * nb) return MRL_ENOSPC;
    a.ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("ddpg.act", -1.0, -1.0, st);
    hipLaunchKernelGGL(ddpg_act_kernel, dim3(nb), dim3(ACT_THREADS), 0, st, a);
    MRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrl_ddpg_store(const mrl_ddpg_desc* d, const mrl_ddpg_state* s, const float* obs0, const float* action,
                              const float* reward, const float* obs1, const uint8_t* terminal1, int n, float reward_scale,
                              void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (n < 1 || !state_ok(s, true) || !obs0 || !action || !reward || !obs1 || !terminal1) return MRL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ddpg_store_kernel, dim3(1), dim3(512), 0, st, *s, d->ob_dim, d->nact, n, obs0, action, reward, obs1,
                       terminal1, reward_scale, d->normalize_observations ? 1 : 0);
    MRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrl_ddpg_perturb(const mrl_ddpg_desc* d, const float* actor, float* perturbed, const float* noise, float stddev,
                                void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (!actor || !perturbed || !noise) return MRL_EINVAL;
    const NetLayout L = actor_layout(d);
    hipLaunchKernelGGL(ddpg_perturb_kernel, dim3((unsigned)std::min<long>((L.P + 255) / 256, 1024)), dim3(256), 0,
                       (hipStream_t)stream, actor, perturbed, noise, stddev, L);
    MRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrl_ddpg_policy_distance(const mrl_ddpg_desc* d, const mrl_ddpg_state* s, const float* perturbed_actor,
                                        const int64_t* idx, int B, float* distance_out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    if (B < 1 || B > 1024) return MRL_EUNSUP;
    if (!state_ok(s, true) || !perturbed_actor || !idx || !distance_out || !workspace) return MRL_EINVAL;
    const NetLayout la = actor_layout(d);
    Carver c{(char*)workspace, 0};
    float* X = c.f((size_t)B * d->ob_dim);
    float* a0 = c.f((size_t)B * d->nact);
    float* a1 = c.f((size_t)B * d->nact);
    float* rs = c.f(2 * (size_t)B);
    Acts st = carve_acts(c, B, la.nh, la.nl, la.ln);
    if (workspace_bytes < c.off) return MRL_ENOSPC;
    hipLaunchKernelGGL(ddpg_distance_kernel, dim3(1), dim3(TRAIN_THREADS), 0, (hipStream_t)stream, *s, la, d->ob_dim, d->nact,
                       B, d->activation, d->normalize_observations ? 1 : 0, perturbed_actor, idx, distance_out, X, a0, a1,
                       rs, st);
    MRL_LAUNCH_CHECK();
    return 0;
}
