// See pixelcnn.h.
#include "pixelcnn.h"
#include <math.h>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

namespace {

constexpr int TILE = PCNN_TILE, NW = PCNN_WAVES, NTHR = 64 * NW;

// ---------------------------------------------------------------------------------------------- the operation tables (host)
struct Builder {
    PcnnPlan& p;
    int W;
    long long slab = 0, packed = 0, params = 0;
    PcnnBuf alloc(int rows, int cols, int ch) {
        PcnnBuf b{(int)slab, rows, cols, ch};
        slab += (long long)rows * cols * TILE * ch;
        return b;
    }
    // a conv of the module (cout, cin, kh, kw), of whose window (origin (r0, c0), kw columns) the first ntaps taps are kept
    void op(PcnnBuf src, PcnnBuf dst, int cin, int cout, int kh, int kw, int r0, int c0, int ntaps, int epi, int pre_relu = 0,
            const PcnnBuf* add = nullptr) {
        PcnnOp o{};
        o.src = src; o.dst = dst;
        if (add) { o.add = *add; o.has_add = 1; }
        o.cin = round_up(cin, 16); o.coutp = round_up(cout, 16);
        o.half = epi == PCNN_EPI_GATE ? cout / 2 : 0;
        o.ntaps = ntaps; o.r0 = r0; o.c0 = c0; o.ncols = kw;
        o.epi = epi; o.pre_relu = pre_relu;
        o.woff = (int)packed; packed += (long long)ntaps * o.cin * o.coutp;
        o.boff = (int)packed; packed += o.coutp;
        o.kh = kh; o.kw = kw; o.cin_real = cin; o.cout_real = cout;
        o.pw = (int)params; params += (long long)cout * cin * kh * kw;
        o.pb = (int)params; params += cout;
        p.ops[p.n_ops++] = o;
    }
};

void build_plan(const PcnnCfg& c, int W, PcnnPlan& p) {
    p.n_ops = 0;
    Builder b{p, W};
    const int hid = c.hid, vc = c.levels * c.channels;
    PcnnBuf last;
    if (!c.gated) {
        // conv1: mask A 7 x 7 keeps 3 rows of 7 and 3 taps of the centre row; blocks: mask B 3 x 3 keeps one row of 3 and 2 taps
        p.image = b.alloc(4, W, PCNN_IMG_CH);
        PcnnBuf cur = b.alloc(2, W, hid);
        b.op(p.image, cur, c.channels, hid, 7, 7, -3, -3, 24, PCNN_EPI_NONE);
        for (int k = 0; k < c.n_blocks; ++k) {
            PcnnBuf nxt = b.alloc(2, W, hid);
            b.op(cur, nxt, hid, hid, 3, 3, -1, -1, 5, PCNN_EPI_RELU);
            cur = nxt;
        }
        last = b.alloc(1, 1, hid);
        b.op(cur, last, hid, hid, 1, 1, 0, 0, 1, PCNN_EPI_RELU);
    } else {
        // a gated block with kernel size k: the vertical conv (k / 2 + 1, k) sees the k / 2 + 1 rows above, the horizontal conv
        // (1, k / 2 + 1) the k / 2 + 1 pixels to the left (CroppedConv2d: padding == kernel size on that side, cropped back)
        p.image = b.alloc(5, W, PCNN_IMG_CH);
        const PcnnBuf bv = b.alloc(1, 1, 2 * hid), bt = b.alloc(1, 1, 2 * hid), bh = b.alloc(1, 1, 2 * hid), bg = b.alloc(1, 1, hid);
        PcnnBuf xin = p.image, hin = p.image;
        int cin = c.channels;
        for (int k = 0; k <= c.n_blocks; ++k) {
            const int ks = k == 0 ? 7 : 3, kv = ks / 2 + 1;
            const PcnnBuf xout = b.alloc(3, W, hid), hout = b.alloc(1, W, hid);
            b.op(xin, bv, cin, 2 * hid, kv, ks, -kv, -(ks / 2), kv * ks, PCNN_EPI_NONE);            // vertical_conv
            b.op(bv, bt, 2 * hid, 2 * hid, 1, 1, 0, 0, 1, PCNN_EPI_NONE);                              // x_to_h_conv
            b.op(bv, xout, 2 * hid, 2 * hid, 1, 1, 0, 0, 1, PCNN_EPI_GATE);                            // vertical_gate_conv, gate
            b.op(hin, bh, cin, 2 * hid, 1, kv, 0, -kv, kv, PCNN_EPI_NONE, 0, &bt);                     // horizontal_conv + x_to_h
            b.op(bh, bg, 2 * hid, 2 * hid, 1, 1, 0, 0, 1, PCNN_EPI_GATE);                              // horizontal_gate_conv, gate
            b.op(bg, hout, hid, hid, 1, 1, 0, 0, 1, PCNN_EPI_NONE, 0, k > 0 ? &hin : nullptr);        // horizontal_output (+ h)
            xin = xout; hin = hout; cin = hid;
        }
        last = b.alloc(1, 1, hid);
        b.op(hin, last, hid, hid, 1, 1, 0, 0, 1, PCNN_EPI_RELU, 1);                                   // conv2(relu(h)), relu
    }
    p.logits = b.alloc(1, 1, round_up(vc, 16));
    b.op(last, p.logits, hid, vc, 1, 1, 0, 0, 1, PCNN_EPI_NONE);                                       // conv4
    p.slab_floats = b.slab; p.packed_floats = b.packed; p.param_floats = b.params;
}

// ---------------------------------------------------------------------------------------------- packing
// flat parameters (per operation: weight (cout, cin, kh, kw), bias) -> [tap][cin / 4][coutp][4] + [coutp].  Only the kept taps
// are packed: that IS the mask, whatever the module's weight holds at the masked entries.
__global__ __launch_bounds__(256) void pcnn_pack_kernel(const float* __restrict__ params, float* __restrict__ packed, PcnnOp op) {
    const int kq = op.cin >> 2;
    const long long nw = (long long)op.ntaps * op.cin * op.coutp;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < nw) {
        const int s = (int)(idx & 3);
        const long long r = idx >> 2;
        const int n = (int)(r % op.coutp);
        const int g = (int)((r / op.coutp) % kq), t = (int)(r / ((long long)op.coutp * kq));
        const int ci = 4 * g + s, ky = t / op.kw, kx = t % op.kw;
        float v = 0.f;
        if (ci < op.cin_real && n < op.cout_real) v = params[op.pw + (((long long)n * op.cin_real + ci) * op.kh + ky) * op.kw + kx];
        packed[op.woff + idx] = v;
    } else if (idx < nw + op.coutp) {
        const int n = (int)(idx - nw);
        packed[op.boff + n] = n < op.cout_real ? params[op.pb + n] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------- the sampler
__device__ __forceinline__ float* at(float* slab, const PcnnBuf& b, int i, int j) {
    const int r = i % b.rows, c = b.cols == 1 ? 0 : j;
    return slab + b.off + (size_t)((r * b.cols + c) * TILE) * b.ch;
}

template <bool GATE>
__device__ __forceinline__ void run_op(const PcnnOp& op, const float* __restrict__ wts, float* slab, int i, int j, int W, int wave,
                                       int lane) {
    const int m = lane & 15, q = lane >> 4;
    const int units = (GATE ? op.half : op.coutp) >> 4;
    const int kq = op.cin >> 2;
    for (int u = wave; u < units; u += NW) {
        const int n = u * 16 + m;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < op.ntaps; ++t) {
            const int ii = i + op.r0 + t / op.ncols, jj = j + op.c0 + t % op.ncols;
            if (ii < 0 || jj < 0 || jj >= W) continue;            // zero padding (ii <= i < H always)
            const float* a = at(slab, op.src, ii, jj) + m * op.src.ch + 4 * q;
            const float* b = wts + op.woff + ((size_t)(t * kq + q) * op.coutp + n) * 4;
            // within a 16-deep step the MFMA s of lane group q consumes channel k0 + 4 q + s on both operands
            for (int k0 = 0; k0 < op.cin; k0 += 16) {
                f32x4 av = *reinterpret_cast<const f32x4*>(a + k0);
                if (op.pre_relu) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) av[s] = fmaxf(av[s], 0.f);
                }
                const float* bk = b + (size_t)(k0 >> 2) * op.coutp * 4;
                const f32x4 bv = *reinterpret_cast<const f32x4*>(bk);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc0, 0, 0, 0);
                if (GATE) {
                    const f32x4 bw = *reinterpret_cast<const f32x4*>(bk + (size_t)op.half * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bw[s], acc1, 0, 0, 0);
                }
            }
        }
        // accumulator: column n, rows (samples) 4 q .. 4 q + 3
        float* d = at(slab, op.dst, i, j);
        const float* ad = op.has_add ? at(slab, op.add, i, j) : nullptr;
        const float bias0 = wts[op.boff + n], bias1 = GATE ? wts[op.boff + op.half + n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int smp = 4 * q + r;
            float v = acc0[r] + bias0;
            if (ad) v += ad[smp * op.add.ch + n];
            if (GATE) v = tanhf(v) * (1.f / (1.f + expf(-(acc1[r] + bias1))));
            else if (op.epi == PCNN_EPI_RELU) v = fmaxf(v, 0.f);
            d[smp * op.dst.ch + n] = v;
        }
    }
}

__global__ __launch_bounds__(NTHR) void pcnn_sample_kernel(const PcnnOp* __restrict__ ops, int n_ops, PcnnBuf image, PcnnBuf logit,
                                                           const float* __restrict__ wts, float* ws, long long slab_floats, int B, int H,
                                                           int W, int C, int V, const float* __restrict__ uniforms,
                                                           const int* __restrict__ given, int n_given, int* __restrict__ levels,
                                                           float* __restrict__ out_image, float* __restrict__ out_logits) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* slab = ws + (size_t)blockIdx.x * (size_t)slab_floats;
    const int b0 = blockIdx.x * TILE, HW = H * W, VC = V * C;
    const float scale = (float)(V - 1);
    for (int p = 0; p < HW; ++p) {
        const int i = p / W, j = p - i * W;
        for (int o = 0; o < n_ops; ++o) {
            const PcnnOp& op = ops[o];
            if (op.epi == PCNN_EPI_GATE) run_op<true>(op, wts, slab, i, j, W, wave, lane);
            else run_op<false>(op, wts, slab, i, j, W, wave, lane);
            __syncthreads();
        }
        // the draw: one thread per (sample, channel); the smallest v with u < CDF_v, clamped to V - 1
        const float* lg = at(slab, logit, 0, 0);
        float* img = at(slab, image, i, j);
        if (tid < TILE * PCNN_IMG_CH) {
            const int smp = tid / PCNN_IMG_CH, c = tid - smp * PCNN_IMG_CH;
            float val = 0.f;                                       // the padding channels of the image cache
            if (c < C) {
                const int b = b0 + smp;
                const bool valid = b < B;                          // a sample past the batch computes like any other, unwritten
                const size_t idx = ((size_t)(valid ? b : 0) * C + c) * HW + p;
                const float* l = lg + smp * logit.ch + c;
                int lev = V - 1;
                if (p < n_given) {
                    lev = valid ? given[idx] : 0;
                    lev = lev < 0 ? 0 : (lev > V - 1 ? V - 1 : lev);
                } else {
                    float mx = l[0];
                    for (int v = 1; v < V; ++v) mx = fmaxf(mx, l[v * C]);
                    float z = 0.f;
                    for (int v = 0; v < V; ++v) z += expf(l[v * C] - mx);
                    const float thr = (valid ? uniforms[idx] : 0.5f) * z;
                    float cum = 0.f;
                    for (int v = 0; v < V; ++v) {
                        cum += expf(l[v * C] - mx);
                        if (thr < cum) lev = min(lev, v);
                    }
                }
                val = (float)lev / scale;
                if (valid) { levels[idx] = lev; out_image[idx] = val; }
            }
            img[tid] = val;
        }
        if (out_logits) {
            for (int e = tid; e < TILE * VC; e += NTHR) {
                const int smp = e / VC, n = e - smp * VC, b = b0 + smp;
                if (b < B) out_logits[((size_t)b * VC + n) * HW + p] = lg[smp * logit.ch + n];
            }
        }
        __syncthreads();
    }
}

std::mutex g_plans_mu;
std::map<std::tuple<int, int, int, int, int, int>, std::unique_ptr<PcnnPlan>> g_plans;

}  // namespace

bool pcnn_cfg_ok(const PcnnCfg& c) {
    return (c.gated == 0 || c.gated == 1) && c.n_blocks >= 0 && c.n_blocks <= PCNN_MAX_BLOCKS && (c.channels == 1 || c.channels == 3) &&
           c.hid >= 16 && c.hid <= PCNN_MAX_HID && c.hid % 16 == 0 && c.levels >= 2 && c.levels <= PCNN_MAX_LEVELS;
}

const PcnnPlan* pcnn_plan(const PcnnCfg& c, int width) {
    std::lock_guard<std::mutex> lk(g_plans_mu);
    auto& slot = g_plans[std::make_tuple(c.gated, c.n_blocks, c.channels, c.hid, c.levels, width)];
    if (!slot) {
        slot.reset(new PcnnPlan());
        build_plan(c, width, *slot);
    }
    return slot.get();
}

size_t pcnn_header_bytes() { return sizeof(PcnnOp) * PCNN_MAX_OPS; }

int launch_pcnn_pack(const PcnnCfg& c, const float* params, float* packed, hipStream_t s) {
    const PcnnPlan* p = pcnn_plan(c, 1);                           // the packed layout does not depend on the width
    for (int o = 0; o < p->n_ops; ++o) {
        const PcnnOp& op = p->ops[o];
        const long long n = (long long)op.ntaps * op.cin * op.coutp + op.coutp;
        MMVAE_LAUNCH(pcnn_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, params, packed, op);
    }
    return mmvae_check_launch("pixelcnn_pack");
}

int launch_pcnn_sample(const PcnnCfg& c, const float* packed, void* ws, int B, int H, int W, const float* uniforms, const int* given,
                       int n_given, int* levels, float* image, float* logits, hipStream_t s) {
    MMVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0,
                  "pixelcnn_sample: the workspace and the packed weights must be 16-byte aligned");
    const PcnnPlan* p = pcnn_plan(c, W);
    // the table rides in the head of the workspace (the plan outlives the copy)
    if (hipMemcpyAsync(ws, p->ops, sizeof(PcnnOp) * p->n_ops, hipMemcpyHostToDevice, s) != hipSuccess) {
        mmvae_set_error("pixelcnn_sample: copying the operation table failed");
        return MMVAE_EHIP;
    }
    float* slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + pcnn_header_bytes());
    MMVAE_LAUNCH(pcnn_sample_kernel, dim3(ceil_div(B, TILE)), dim3(NTHR), 0, s, reinterpret_cast<const PcnnOp*>(ws), p->n_ops, p->image,
                 p->logits, packed, slabs, p->slab_floats, B, H, W, c.channels, c.levels, uniforms, given, n_given, levels, image, logits);
    return mmvae_check_launch("pixelcnn_sample");
}
