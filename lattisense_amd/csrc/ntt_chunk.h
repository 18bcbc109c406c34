// ntt_chunk.h — how launch_ntt cuts a batch into chunks (lsa_set_ntt_chunk_mib) and what a chunk's launches take as their
// arguments.  Plain C++ over NttPassArgs: the launcher, the CPU replay (emu_ntt.cpp) and tests/cpp/test_ntt_chunk.cpp share it.
#pragma once
#include "ntt_core.h"

// batch items per chunk: as many as fit `mib` MiB of active limbs (8 n bytes each, active_rows per item), at least one, at
// most the batch; mib <= 0: the whole batch in one chunk
inline int ntt_chunk_items(int n, int active_rows, int batch, int mib) {
    if (mib <= 0) return batch;
    const long long per_item = 8LL * n * (active_rows > 1 ? active_rows : 1);
    long long fit = ((long long)mib << 20) / per_item;
    if (fit > batch) fit = batch;
    return (int)(fit < 1 ? 1 : fit);
}

// The arguments of the chunk that starts at batch item b0, from the whole batch's.  A chunk's workgroups count their batch index
// from 0 (ntt_decode_block), and every fix-up function addresses a fused operand as base + b * stride, so EVERY operand that
// has a batch stride moves by b0 items of its own stride, whatever the fusion kind: the accumulators, bases, outputs, the
// rescale heads' last limb, the plaintexts and the product's second factor.  A null operand stays null; a shared one (stride
// 0) stays where it is.  fz_k / fz_k2 (one constant per limb), fz_scatter (one index map) and the tables have no batch
// dimension and are left alone, and so is everything else: src, dst and batch are the launcher's to set per pass.
inline NttPassArgs ntt_chunk_rebase(const NttPassArgs& whole, int b0) {
    NttPassArgs a = whole;
    if (a.fz_a) a.fz_a += (long long)b0 * a.fz_a_stride;
    if (a.fz_b) a.fz_b += (long long)b0 * a.fz_b_stride;
    if (a.fz_base) a.fz_base += (long long)b0 * a.fz_base_stride;
    if (a.fz_out) a.fz_out += (long long)b0 * a.fz_out_stride;
    if (a.fz_last) a.fz_last += (long long)b0 * a.fz_last_stride;
    if (a.fz_pt) a.fz_pt += (long long)b0 * a.fz_pt_stride;
    return a;
}
