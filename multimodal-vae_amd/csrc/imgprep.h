// Scale(S) + CenterCrop(S) + ToTensor of a ragged batch of decoded RGB images on the device, bit for bit Pillow's 8-bit bilinear
// resample (imgprep_core.h states the arithmetic and the limits).
//
// imgprep_kernel: one workgroup of IMGPREP_THREADS per image.  The workgroup first checks the image's descriptor (sides, offset, span
// against pixels_bytes) and refuses an unusable one before reading a byte of it: zeros, status -1.  Then, in LDS:
//   - per axis the S spans of the crop window (first tap, tap count, weight sum) and, when S x most taps <= COEF_CAP, the int32
//     coefficients themselves; a larger table is not kept and its coefficients are computed where they are used, by the same function;
//   - bands of output rows: the input rows a band depends on are staged STAGE_BYTES at a time with aligned dword loads along the row
//     (only the columns the crop window depends on; a dword that leaves [pixels, pixels + pixels_bytes) is read byte by byte, inside
//     it).  The loads of a round are issued together into registers, and those of the next round while this round is resampled.  The
//     horizontal pass writes rows x S x 3 bytes of 8-bit intermediate (at most LDS_BUDGET), and the vertical pass reads that and
//     stores the band planar, uint8 and / or float32.
// LDS is sizeof(Lds) = 101 KB, dynamic: one workgroup per CU.
// A byte of the output belongs to one lane, the passes are separated by barriers, and there is no atomic: two calls give identical
// bits, and an image's result does not depend on the batch it is in.
#pragma once
#include "common.h"
#include "imgprep_core.h"

enum { IMGPREP_THREADS = 1024 };

int launch_imgprep_scale_crop(const uint8_t* pixels, long long pixels_bytes, const long long* offsets, const int* heights, const int* widths,
                              int n, int S, uint8_t* out_u8, float* out_f32, int* status, hipStream_t st);
