// Geometry of the half-image forms of the thin MultiMNIST kernels (conv1.hip's forward, dec_last.hip's training form): which
// pixels a workgroup owns, which image rows it stages, and its LDS map.  Plain C++17 (no HIP): the kernels and tests/host/thin_split_geo_check.cpp read the same
// numbers, the program walks every address on the CPU.
//
// conv1 (Conv2d(1, 32, 4, 2, 1), 50x50 -> 25x25): the 625 output pixels are 20 tiles of 32 rows of the patch matrix (640 rows, 15
// of padding).  Workgroup z of an image owns tiles [10z, 10z + 10), i.e. pixels [320z, 320z + 320) of the image -- output rows 0..12
// (row 12 up to column 19) and 12..24 -- and stages the 28 image rows 2*oy - 1 .. 2*oy + 2 those pixels read, row -1 / 50 as zeros.
#pragma once

namespace c1s {

constexpr int IMG = 50, OH = 25, NPIX = 625, C = 32;
constexpr int HALVES = 2, TILES = 10, PIX = TILES * 32;        // tiles / patch-matrix rows of one workgroup
constexpr int IROWS = 28;               // staged image rows
constexpr int IW = 54;                  // bf16 per staged row: image column x at index x + 2 (a pair of columns is one aligned word),
                                        // index 1 and 52 the zero halo, 0 and 53 unused (zeroed)
constexpr int PP = 48;                  // patches: bytes per pixel (16 bf16 + 16)

constexpr int pix0(int z) { return z * PIX; }                                           // first owned pixel
constexpr int npix(int z) { return NPIX - pix0(z) < PIX ? NPIX - pix0(z) : PIX; }        // owned pixels (the rest of the 320 rows: zero)
constexpr int oy_lo(int z) { return pix0(z) / OH; }
constexpr int oy_hi(int z) { return (pix0(z) + npix(z) - 1) / OH; }
constexpr int y0(int z) { return 2 * oy_lo(z) - 1; }                                     // image row of staged row 0
constexpr int ld_row0(int z) { return y0(z) < 0 ? 0 : y0(z); }                           // first image row that is loaded
constexpr int ld_rows(int z) { return (y0(z) + IROWS - 1 > IMG - 1 ? IMG - 1 : y0(z) + IROWS - 1) - ld_row0(z) + 1; }
constexpr int pad_row(int z) { return y0(z) < 0 ? 0 : IROWS - 1; }                       // the staged row outside the image
constexpr int LD_ROWS = 27, LD_VEC = LD_ROWS * (IMG / 2);                                // 8-byte vectors a workgroup loads

// staged cell (bf16 index) of image position (y, x), x in [-1, 50]
constexpr int cell(int z, int y, int x) { return (y - y0(z)) * IW + x + 2; }
// first cell of the 4x4 window of local pixel lp, kernel rows 2*half, 2*half + 1
constexpr int window(int z, int lp, int half) {
    return cell(z, 2 * ((pix0(z) + lp) / OH) - 1 + 2 * half, 2 * ((pix0(z) + lp) % OH) - 1);
}

static_assert(pix0(0) == 0 && pix0(1) == npix(0) && pix0(1) + npix(1) == NPIX && HALVES == 2, "the halves partition the 625 pixels");
static_assert(2 * oy_hi(0) + 2 <= y0(0) + IROWS - 1 && 2 * oy_hi(1) + 2 <= y0(1) + IROWS - 1, "staged rows cover every row a window reads");
static_assert(ld_rows(0) == LD_ROWS && ld_rows(1) == LD_ROWS, "both halves load 27 image rows");
static_assert((ld_row0(0) * IMG) % 2 == 0 && (ld_row0(1) * IMG) % 2 == 0 && (IMG * IMG) % 2 == 0 && IMG % 2 == 0,
              "8-byte vectors: a half starts on an even float of an image, an image on an even float of the batch, a vector stays in its row");
static_assert(y0(0) + pad_row(0) == -1 && y0(1) + pad_row(1) == IMG, "exactly one staged row of each half lies outside the image");
static_assert((IW * 2) % 4 == 0, "a pair of columns is one aligned 4-byte word of LDS");

constexpr int IMG_BYTES = (IROWS * IW * 2 + 15) / 16 * 16;
constexpr int HALF_CU = 160 * 1024 / 2;

// forward: 4 waves
constexpr int F_WAVES = 4, F_NTHR = F_WAVES * 64;
constexpr int F_OFF_IMG = 0, F_OFF_PAT = F_OFF_IMG + IMG_BYTES, F_OFF_SCR = F_OFF_PAT + PIX * PP, F_LDS = F_OFF_SCR + F_WAVES * 2560;
static_assert(F_LDS <= HALF_CU, "conv1 forward: two workgroups per CU");

}  // namespace c1s

// Decoder tail (ConvTranspose2d(32, 1, 4, 2, 1), 25x25x32 -> 50x50): workgroup z of an image owns input rows [0, 13) or [13, 25) and
// the output rows 2*iy, 2*iy + 1 of those, [0, 26) or [26, 50).  It stages its rows and one halo row on each side (rows outside
// the image as zeros), makes P[pixel][tap] for the staged rows, the logits of the output rows 2*lo - 1 .. 2*hi the 4x4 gradient
// windows of its own pixels touch (the outer two for the gradient only), and patches / input gradient / weight-gradient partial
// for its own pixels.
namespace dls {

constexpr int IH = 25, IW = 25, OH = 50, OW = 50, C = 32, NPIX = IH * IW;
constexpr int HALVES = 2;
constexpr int own_lo(int z) { return z ? 13 : 0; }
constexpr int own_hi(int z) { return z ? IH : 13; }                          // exclusive
constexpr int own_pix(int z) { return (own_hi(z) - own_lo(z)) * IW; }        // 325 / 300
constexpr int own_tiles(int z) { return (own_pix(z) + 31) / 32; }            // 11 / 10
constexpr int st_lo(int z) { return own_lo(z) - 1; }                         // first staged input row (-1 / 12)
constexpr int st_rows(int z) { return own_hi(z) - own_lo(z) + 2; }           // 15 / 14
constexpr int st_pix(int z) { return st_rows(z) * IW; }                      // 375 / 350
constexpr int st_tiles(int z) { return (st_pix(z) + 31) / 32; }              // 12 / 11
constexpr int lo_lo(int z) { return 2 * own_lo(z) - 1; }                     // first output row of the dlogit buffer (-1 / 25)
constexpr int lo_rows(int z) { return 2 * (own_hi(z) - own_lo(z)) + 2; }     // 28 / 26
constexpr int out_lo(int z) { return 2 * own_lo(z); }                        // owned output rows [out_lo, out_hi)
constexpr int out_hi(int z) { return 2 * own_hi(z); }
constexpr int ST_ROWS_MAX = 384, OWN_ROWS_MAX = 352, LO_ROWS_MAX = 28;       // pixel rows of A / P, of the patches; dlogit rows
constexpr int AP = 80;                  // A tile: bytes per pixel (32 bf16 + 16)
constexpr int PP = 48;                  // patches: bytes per pixel (16 bf16 + 16)
constexpr int DLW = 52;                 // dlogit row: output column ox at index ox + 1, zero halo at 0 and 51
constexpr int SCR = 2560;               // epilogue scratch of one wave (convres_epi.h)
constexpr int MAX_WAVES = 8;

// staged pixel row of input pixel (iy, ix); owned pixel j of the workgroup is staged pixel j + IW
constexpr int st_pixel(int z, int iy, int ix) { return (iy - st_lo(z)) * IW + ix; }
// dlogit cell of output position (oy, ox), ox in [-1, 50]
constexpr int dl_cell(int z, int oy, int ox) { return (oy - lo_lo(z)) * DLW + ox + 1; }
// first dlogit cell of the 4x4 window of owned pixel j, kernel rows 2*half, 2*half + 1
constexpr int dl_window(int z, int j, int half) { return dl_cell(z, 2 * (own_lo(z) + j / IW) - 1 + 2 * half, 2 * (j % IW) - 1); }

static_assert(own_lo(0) == 0 && own_hi(0) == own_lo(1) && own_hi(1) == IH, "the owned input rows partition [0, 25)");
static_assert(out_lo(0) == 0 && out_hi(0) == out_lo(1) && out_hi(1) == OH, "the owned output rows partition [0, 50)");
static_assert(st_lo(0) <= own_lo(0) - 1 && st_lo(0) + st_rows(0) >= own_hi(0) + 1 && st_lo(1) <= own_lo(1) - 1 && st_lo(1) + st_rows(1) >= own_hi(1) + 1,
              "one halo row on each side");
// logit row oy reads input rows (oy + 1) / 2 and (oy + 1) / 2 - 1
static_assert((lo_lo(0) + 1) / 2 - 1 >= st_lo(0) && (lo_lo(0) + lo_rows(0)) / 2 < st_lo(0) + st_rows(0) &&
              (lo_lo(1) + 1) / 2 - 1 >= st_lo(1) && (lo_lo(1) + lo_rows(1)) / 2 < st_lo(1) + st_rows(1), "staged rows cover every row a logit reads");
// the window of owned pixel row iy reads dlogit rows 2*iy - 1 .. 2*iy + 2
static_assert(2 * own_lo(0) - 1 >= lo_lo(0) && 2 * (own_hi(0) - 1) + 2 < lo_lo(0) + lo_rows(0) &&
              2 * own_lo(1) - 1 >= lo_lo(1) && 2 * (own_hi(1) - 1) + 2 < lo_lo(1) + lo_rows(1), "the dlogit rows cover every row a window reads");
static_assert(st_tiles(0) * 32 <= ST_ROWS_MAX && st_tiles(1) * 32 <= ST_ROWS_MAX && own_tiles(0) * 32 <= OWN_ROWS_MAX && own_tiles(1) * 32 <= OWN_ROWS_MAX &&
              lo_rows(0) <= LO_ROWS_MAX && lo_rows(1) <= LO_ROWS_MAX, "buffer extents");
static_assert(OWN_ROWS_MAX + IW + 4 <= ST_ROWS_MAX, "the weight gradient reads A at owned row + 25 (+ 4: transposed pair) inside the tile");
static_assert((IW * AP) % 16 == 0, "the owned pixels start on a 16-byte boundary of A");

// LDS map.  P (fp32 [384][16]) is dead when the patches ([352][48] bf16) are written over it; the dlogit buffer is dead (last read:
// the patches pass, a barrier behind it) when the waves' epilogue scratch, later their weight-gradient partials, take its place.
constexpr int OFF_A = 0;
constexpr int OFF_P = OFF_A + ST_ROWS_MAX * AP;
constexpr int P_BYTES = ST_ROWS_MAX * 64;
constexpr int OFF_DL = OFF_P + P_BYTES;
constexpr int DL_BYTES = LO_ROWS_MAX * DLW * 4;
constexpr int SCR_BYTES = MAX_WAVES * SCR;
constexpr int OFF_TAB = OFF_DL + (DL_BYTES > SCR_BYTES ? DL_BYTES : SCR_BYTES);
constexpr int LDS = OFF_TAB + 2 * C * 8;
constexpr int STATIC_LDS = MAX_WAVES * 4 + MAX_WAVES * C * 8;                  // the waves' loss partials and BatchNorm-backward sums
static_assert(OWN_ROWS_MAX * PP <= P_BYTES, "the patches reuse the P buffer");
static_assert(MAX_WAVES * C * 16 * 4 <= SCR_BYTES, "the weight-gradient partials reuse the epilogue scratch");
static_assert(OFF_P % 16 == 0 && OFF_DL % 16 == 0 && OFF_TAB % 16 == 0, "16-byte aligned regions");
static_assert(LDS <= (160 * 1024 - STATIC_LDS) / 2, "two workgroups per CU");
// phases of a workgroup (separated by barriers) and what is live in each: 0 stage (A, dlogit <- targets), 1 forward (A -> P),
// 2 logits (P -> dlogit), 3 patches (dlogit -> patches), 4 input gradient (patches, scratch), 5 weight gradient (A, patches ->
// partials in the scratch), 6 partial sum
constexpr int P_LAST = 2, PAT_FIRST = 3, DL_LAST = 3, SCR_FIRST = 4;
static_assert(P_LAST < PAT_FIRST && DL_LAST < SCR_FIRST, "regions that share space are never live together");

}  // namespace dls
