// The library's knobs: named process-wide integers that a test, a tool or bench.py --knob sets through mmvae_debug_set
// (include/mmvae_hip.h) and a launcher reads with mmvae_knob(K_name).  THIS table is the complete list and the one home of every
// default; a name it lacks does not compile on the C++ side and is MMVAE_EINVAL at the C boundary.
//   KNOB(name, default, kind, "meaning, with the values it takes")
// kind (nothing on the launch path reads it):
//   AB       same results, another route: the older or alternative form of a kernel, a launch order, a stream assignment
//   TUNE     a size or a count, same results
//   MEASURE  results WRONG by design: part of the work is left out so that the rest can be timed
//   ADDR     the low / high 32 bits of a device pointer (mmvae_knob_ptr): where a kernel writes its phase time stamps, 0 / 0 = nowhere
// A knob is read when a launch is issued, so a captured graph keeps the value it was captured with.
#pragma once
#include <atomic>

#define MMVAE_KNOBS(KNOB) \
    KNOB(convres, 1, AB, "image-resident conv kernels (convres.hip); 0: every layer on gemm_gather, except launches with a staging transform, which exist only there") \
    KNOB(convres_celeba, 1, AB, "convres.hip on the 64x64 image tower's layers (CelebA, COCO); 0: those layers on gemm_gather") \
    KNOB(convres_alt, 0, AB, "convres.hip tile configurations: 1 hallucinate.6 with 4 images per workgroup, 3 no direct-B kernels, 4 no split bottleneck kernels, 5 no 16-image hallucinate.0") \
    KNOB(convres_dbg, 0, MEASURE, "convres kernels leave phases out (bit mask, tools/convres_check.py)") \
    KNOB(convres_ts_lo, 0, ADDR, "convres kernels: time stamps of workgroup 0's phases, low half of the pointer") \
    KNOB(convres_ts_hi, 0, ADDR, "high half") \
    KNOB(mm_fuse_bn, 1, AB, "MultiMNIST step: BatchNorm passes folded into the staging of the image-resident conv kernels; 0: the unfused bn_act + gather-GEMM chain") \
    KNOB(ca_fuse_bn, 1, AB, "the same for the 64x64 image tower (CelebA, COCO)") \
    KNOB(mm_stage_out, 1, AB, "the staging conv kernels leave the activated operand / BatchNorm-backward dr behind for the weight gradient; 0: materialised on the side stream in front of it") \
    KNOB(mm_conv1_mfma, 1, AB, "MultiMNIST features.0 forward and weight gradient on conv1.hip; 0: gemm_gather") \
    KNOB(dec_last_mfma, 1, AB, "MultiMNIST decoder tail (hallucinate.9 + BCE + its gradients) on dec_last.hip; 0: separate launches") \
    KNOB(dec_last_ca, 1, AB, "the 64x64 tower's decoder tail on dec_last.hip; 0: separate launches") \
    KNOB(dec_last_ca_dbg, 0, MEASURE, "64x64 decoder tail leaves work out: bit 0 logits, 1 patches, 2 input gradient, 3 weight gradient, 4 P") \
    KNOB(wgrad_ring, 1, AB, "ring-staged weight-gradient kernels (wgrad_ring.hip); 0: the streamed gemm_gather form") \
    KNOB(wr_pair, 0, AB, "1: the two-classes-per-workgroup geometries of wgrad_ring.hip (tried and lost, DESIGN)") \
    KNOB(wr_wgs, -1, TUNE, "workgroups of a ring launch in quarters of the CU count; -1: 4 from 4e9 MACs, else 3") \
    KNOB(wr_wgs_big, 0, TUNE, "the same for a geometry that names its own (G::WGQ); 0: the geometry's") \
    KNOB(wr_bias, 6, TUNE, "fixed cost of a batch for a ring workgroup, in column tiles, when image groups are dealt to classes") \
    KNOB(wr_run, 0, TUNE, "consecutive jobs dealt to one XCD residue by the ring launch's workgroup order; 0: one per job class and channel slice") \
    KNOB(wr_xcd, 1, AB, "0: ring jobs in sorted order, not dealt to the XCDs") \
    KNOB(wr_atomic_kb, 256, TUNE, "a ring launch adds into the packed gradient by fp32 atomics up to this many KB of dW; above: partial copies + reduce") \
    KNOB(wr_dbg, 0, MEASURE, "ring kernels leave phases out (bit mask, tools/wgrad_check.py)") \
    KNOB(wr_ts_lo, 0, ADDR, "ring kernels: time stamps of workgroup 0's phases, low half of the pointer") \
    KNOB(wr_ts_hi, 0, ADDR, "high half") \
    KNOB(wgrad_atomic, 0, AB, "1: streamed weight gradients add into the packed gradient by fp32 atomics, no slab / reduce") \
    KNOB(batch_reduce, 1, AB, "one reduce launch per flushed side stream; 0: one behind every weight gradient") \
    KNOB(mm_wgrad_inline, 0, AB, "1: MultiMNIST image weight gradients on the main stream (no fork, no join); 2: and their partial copies summed by one launch in front of the optimizer") \
    KNOB(one_wgrad_stream, 0, AB, "1: one weight-gradient side stream instead of two") \
    KNOB(side_lanes, 3, AB, "bit 0: lane-1 side work goes to the second-modality stream; bit 1: lane 2 to the spare weight-gradient stream") \
    KNOB(mm_cls_lane, 1, AB, "side-stream lane of the classifier's grouped weight gradients") \
    KNOB(mm_conv3_lane, 0, AB, "side-stream lane of features.5's weight gradient") \
    KNOB(mm_conv4_lane, 0, AB, "side-stream lane of features.8's weight gradient") \
    KNOB(mm_forks, 0, AB, "1: one fork for the whole encoder / decoder backward instead of one per flush point") \
    KNOB(one_join, -1, AB, "end of step: 1 the side streams meet on one of them and the main stream waits once, 0 it waits for each; -1: once when there are two weight-gradient streams") \
    KNOB(ev_flags, 2, AB, "flags of the step's events: 2 no system-scope fence, 0 HIP's default fence (read when an event is created)") \
    KNOB(no_stop_events, 0, AB, "1: forks are event records on the main stream, not the producer kernel's completion signal") \
    KNOB(adam_blocks, 512, TUNE, "workgroup cap of the Adam kernel") \
    KNOB(begin_blocks, 2048, TUNE, "zero / random-number workgroup cap of the step prologue") \
    KNOB(mm_dz_event, 1, AB, "the main chain joins the text decoder backward on that kernel's own event; 0: on everything enqueued on its stream") \
    KNOB(mm_stage_begin, 1, AB, "staged prologue: the main stream refreshes only what the image encoder's forward reads, the rest on the second-modality stream; 0: one launch") \
    KNOB(mm_early_adam, 1, AB, "the decoders' Adam update runs beside the encoders' backward when the caller passes early_adam; 0: never") \
    KNOB(mm_image_waist, -1, AB, "image-only MultiMNIST step: 1 / 0 the one-expert waist kernels on / off where compiled; -1: the size's default (1 at n_latents = 20, 0 at 100)") \
    KNOB(mnist_strip, -1, AB, "image-only MNIST step: 1 / 0 the column-strip Linear + BatchNorm kernels on / off up to 512 rows; -1: the default, 1") \
    KNOB(text_fwd2, 1, AB, "MultiMNIST text decoder forward: the weights-resident text_decoder_fwd2_kernel at the reference's sizes; 0: the streamed form at every size") \
    KNOB(txt_ts_lo, 0, ADDR, "text decoder forward: time stamps of workgroup 0's phases, low half of the pointer") \
    KNOB(txt_ts_hi, 0, ADDR, "high half") \
    KNOB(pack_runs, 1, AB, "every weight pack: the lanes of a wave walk the source's contiguous direction (pack_geo.h); 0: the row-major assignment it replaced, reference of tests/test_gpu_pack_runs.py") \
    KNOB(pack_stage_grid, 1, AB, "a staged prologue launch holds only its own descriptors' workgroups and the zero / random workgroups it needs; 0: the whole table and begin_blocks workgroups in every launch") \
    KNOB(gemm_small_prefetch, 2, AB, "gemm_small_kernel with 2 .. 4 64-deep chunks of both operands in flight per wave; 0: gemm_small_kernel_v0, reference of tests/test_gpu_gemm_small_forms.py") \
    KNOB(dbg_skip_wgrad, 0, MEASURE, "the step without weight gradients: 1 all, 2 ring-staged, 3 streamed, 4 grouped") \
    KNOB(dbg_skip_text, 0, MEASURE, "1: the step without its text kernels") \
    KNOB(dbg_skip_edges, 0, MEASURE, "the step without event edges: 1 all, 2 forks (main -> side), 3 joins") \
    KNOB(dbg_begin_skip, 0, MEASURE, "prologue without: bit 0 the pack, 1 the random draws, 2 the workspace zeroing") \
    KNOB(dbg_begin_skip_zero, 0, MEASURE, "prologue without zeroing: bit 0 the packed gradient, 1 the gradients") \
    KNOB(dbg_text_rows_div, 0, MEASURE, "n > 0: the text decoder on 1/n of its rows") \
    KNOB(coco_cluster, 8, AB, "ranks per 16-row block of the caption decoder's persistent launches: 8, 4, or 0 / 1 one workgroup per block") \
    KNOB(coco_enc_streamed, 0, AB, "1: the caption encoder's weight-streaming kernels instead of the weight-resident ones") \
    KNOB(coco_no_comb, 0, AB, "1: the cluster-of-8 decoder's three-exchange kernels instead of the composed two-exchange form") \
    KNOB(coco_no_comb_bwd, 0, AB, "1: the composed form off in the decoder's backward only") \
    KNOB(coco_no_mse_fuse, 0, AB, "1: the caption MSE not fused into the composed decoder forward") \
    KNOB(coco_module_bf16, 0, AB, "caption module entry points: 0 the fp32 kernels; 1 the step's bf16 persistent kernels on the module's B rows; 2 their forward without saving, backward refuses") \
    KNOB(celeba_layer_mask, 0, AB, "mmvae_celeba_bench_layer: 1 the dropout keep flags take part in the fc layers") \
    KNOB(coco_layer_mask, 0, AB, "mmvae_coco_bench_layer: 1 the dropout keep flags in m1 / m2 take part in the fc layers")

enum MmvaeKnob {
#define KNOB(name, dflt, kind, doc) K_##name,
    MMVAE_KNOBS(KNOB)
#undef KNOB
    K_COUNT
};

extern std::atomic<int> g_mmvae_knobs[K_COUNT];         // util.cpp, initialised to the defaults
static inline int mmvae_knob(MmvaeKnob k) { return g_mmvae_knobs[k].load(std::memory_order_relaxed); }
// the device pointer a pair of ADDR knobs holds
static inline unsigned long long* mmvae_knob_ptr(MmvaeKnob lo, MmvaeKnob hi) {
    return reinterpret_cast<unsigned long long*>(((unsigned long long)(unsigned)mmvae_knob(hi) << 32) | (unsigned)mmvae_knob(lo));
}
