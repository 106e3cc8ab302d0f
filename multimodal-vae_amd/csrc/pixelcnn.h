// Incremental sampler for PixelCNN / GatedPixelCNN (coco/model.py:405-585): the whole H x W raster loop in ONE launch.
//
// The networks are causal, so at pixel (i, j) every layer needs only its activation at (i, j), computed from activations of the
// layer below at raster-earlier positions.  A workgroup owns a tile of PCNN_TILE samples (samples never interact), loops over the
// pixels and, per pixel, over a table of layer operations:
//     gather the taps of a cached layer -> product with one packed weight matrix -> epilogue
// on v_mfma_f32_16x16x4_f32 (M = the tile's samples, N = 16 output channels, K = taps x input channels), fp32 storage and fp32
// accumulation throughout, accurate expf / tanhf.  PixelCNN and GatedPixelCNN are two tables for the same kernel.
//
// Caches (per tile, in the workspace): a layer that is read at other positions keeps a ring of its last rows -- (row reach of its
// reader) + 1, because row i is written while row i - reach is still read further right -- of W columns; a layer that is read only
// at the current pixel keeps that pixel alone.  Every element is [sample][channel], channel fastest.  A tap outside the image is
// skipped (zero padding: it contributes nothing, the bias still applies), so no unwritten element is ever read and the workspace
// needs no initialisation.
//
// A call is ONE sampling kernel; in front of it on the same stream go a copy of the operation table (a few KB, host to device)
// into the head of the workspace and, because the weights are packed on every call, one small packing kernel per layer.
//
// Synchronisation is the workgroup barrier between two operations; there is no grid-wide barrier and every loop has a fixed trip
// count.  A sample's results are a function of (weights, its uniforms, its given pixels, n_given) alone: an MFMA row depends on
// its own A row only, so neither B nor the tile a sample lands in changes a bit.
#pragma once
#include "common.h"

enum {
    PCNN_TILE = 16,          // samples per workgroup: the M of the MFMA
    PCNN_WAVES = 8,          // waves per workgroup; a wave owns whole 16-channel output tiles
    PCNN_MAX_HID = 128,
    PCNN_MAX_SIDE = 64,
    PCNN_MAX_BLOCKS = 15,
    PCNN_MAX_LEVELS = 256,
    PCNN_MAX_OPS = 100,      // gated: 6 per block x 16 blocks + conv2 + conv4
    PCNN_IMG_CH = 16,        // the image's 1 or 3 channels, zero-padded to one 16-deep MFMA step
};
enum { PCNN_EPI_NONE = 0, PCNN_EPI_RELU = 1, PCNN_EPI_GATE = 2 };

struct PcnnCfg { int gated, n_blocks, channels, hid, levels; };

// one cached layer of a tile: element (row, col, sample, ch) at off + (((row % rows) * cols + (cols == 1 ? 0 : col)) * 16 + sample) * ch
struct PcnnBuf { int off, rows, cols, ch; };

struct PcnnOp {
    PcnnBuf src, dst, add;   // add: summed at the current pixel before the epilogue (x_to_h, the residual), when has_add
    int cin, coutp;          // padded to 16; a gate computes coutp = 2 * half columns and stores half
    int half;
    int ntaps, r0, c0, ncols;  // tap t reads (i + r0 + t / ncols, j + c0 + t % ncols): a mask keeps the FIRST ntaps of the window
    int epi, pre_relu, has_add;
    int woff, boff;          // packed: [tap][cin / 4][coutp][4] weights, [coutp] bias
    int kh, kw, cin_real, cout_real, pw, pb;   // the module's (cout, cin, kh, kw) weight and bias in the flat parameter vector
    int pad_[2];
};
static_assert(sizeof(PcnnOp) == 128, "PcnnOp");

struct PcnnPlan {
    PcnnOp ops[PCNN_MAX_OPS];
    int n_ops;
    long long slab_floats;   // workspace floats of one tile
    long long packed_floats, param_floats;
    PcnnBuf image, logits;
};

bool pcnn_cfg_ok(const PcnnCfg& c);
// the table for a width (buffer sizes depend on it); the returned plan lives for the rest of the process
const PcnnPlan* pcnn_plan(const PcnnCfg& c, int width);
size_t pcnn_header_bytes();
int launch_pcnn_pack(const PcnnCfg& c, const float* params, float* packed, hipStream_t s);
int launch_pcnn_sample(const PcnnCfg& c, const float* packed, void* ws, int B, int H, int W, const float* uniforms, const int* given,
                       int n_given, int* levels, float* image, float* logits, hipStream_t s);
