// MultiMNIST canvases made on the device (multimnist/datasets.py): 0 .. 4 MNIST digits, each bilinearly resized (Pillow's 8-bit
// resample, bit for bit) and placed on a 50 x 50 canvas, a canvas whose sum passes 255 drawn again.  Integer arithmetic and a
// counter-based generator only: mmgen_core.h states the resize, the draws and the bounds, and a canvas is a function of (seed, its
// global index, the mode) alone, whatever the batch it is generated in.
//
// mmgen_kernel: one workgroup of MMGEN_THREADS per canvas.  The digit (784 B), the side's coefficient rows, the 28 x s intermediate
// and the canvas as int32 sums sit in LDS (about 13 KB).  Every lane derives the same draws, so the attempt loop is uniform; the
// rejection test is a max over the canvas (wave shuffles, then one LDS word per wave).  A pixel of the canvas belongs to one lane per
// digit and digits are separated by barriers: no atomics on values.  The accepted canvas leaves as 625 dwords (uint8) and / or 625
// float4 (u8 / 255, IEEE division).  The loop is bounded by MAX_ATTEMPTS x 4 x MAX_REDRAWS draws: the kernel always terminates, and
// a canvas that ran out of attempts is written as zeros with FILL text, attempts = 0, and counted in *fail_count (one device atomic
// on that path only).
// mmgen_render_kernel: the same render path from an explicit (n, 4, 4) int32 table (digit index or -1, side, top, left): no draws,
// no rejection; the sum is clamped to 255 and overflow[i] says whether that happened.  A slot outside [index < M, SIDE_MIN <= side <=
// SIDE_MAX, 0 <= top, left, top + side <= 50, left + side <= 50] is never rendered: the canvas is zeros and overflow[i] = -1.
#pragma once
#include "common.h"
#include "mmgen_core.h"

enum { MMGEN_THREADS = 256 };

int launch_mmgen_generate(const uint8_t* digits, const long long* labels, int M, const int32_t* tables, int flags, int min_digits,
                          int max_digits, unsigned long long seed, unsigned long long first, int n, uint8_t* images_u8, float* images_f32,
                          long long* text, int* params, int* attempts, int* fail_count, hipStream_t st);
int launch_mmgen_render(const uint8_t* digits, int M, const int32_t* tables, const int* params, int n, uint8_t* images_u8,
                        float* images_f32, int* overflow, hipStream_t st);
