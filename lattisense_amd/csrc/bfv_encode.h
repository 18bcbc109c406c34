// bfv_encode.h — the BFV slot encoder on the device (lsa_bfv_encode; code in bfv_encode.hip).  `batch` vectors of N integers in
// [0, t) -- row 0 of the 2 x N/2 slot matrix, then row 1 -- become plaintexts in one of three forms:
//   BFV_PT_RINGT  ring-t coefficients [N], words in [0, t): the operand launch_lift_ringt reads
//   BFV_PT_MUL    pt_mul [level+1][N]: NTT domain, Montgomery form, the operand of the lsa_bfv_*_plain_mul entry points
//   BFV_PT_EXT    extended [level+1+k][N] over Q_level u P: NTT domain, plain residues, the operand of the BFV linear transform
// The coefficients are oracle/client.py Client.bfv_encode's: the values placed through Lattigo's batching index matrix, then the
// inverse negacyclic transform mod t with psi_t = g^((t-1)/2N), g the smallest generator of Z_t^*.  The lift to the chain is
// the pt_mul convention of the project: the coefficient in [0, t) is used as it is at every modulus (t is below every q_j and
// p_i), so every residue row starts from the same N words -- the forward transforms read the one coefficient row through the
// single-source lift prologue (NttFusion::pro = 4); no [rows][N] copy of it is ever stored.
//
// The transform mod t is k_bfv_encode_t: one 1024-thread workgroup per plaintext, the whole plaintext as 32-bit words in LDS
// (4.5 N bytes with the padding below: 144 KiB of the 160 KiB per CU at N = 2^15, the kernel's limit).  ABOVE N = 2^15 THE IMAGE
// DOES NOT FIT: the transform then runs on the host (BfvEncodeTables::encode, the routine the kernel's tables come from) and the
// device takes over from the coefficient row.
#pragma once
#include "lsa_internal.h"

namespace lsa {

enum BfvPtForm { BFV_PT_RINGT = 0, BFV_PT_MUL = 1, BFV_PT_EXT = 2 };

#define LSA_BFV_ENC_THREADS 1024
#define LSA_BFV_ENC_MAX_LOGN 15   // the LDS image of k_bfv_encode_t: 4.5 N bytes
#define LSA_BFV_ENC_MIN_LOGN 6    // its first pass works on 32-word chunks, its last on pairs per thread

// rows of a plaintext of this form at `level`
inline int bfv_pt_rows(const Context& c, int level, int form) { return form == BFV_PT_RINGT ? 1 : level + 1 + (form == BFV_PT_EXT ? c.np : 0); }

// the context's encoder tables (built on first use; LSA_ERR_ARG, prefixed by `who`, when t does not allow slot encoding)
const BfvEncodeTables& bfv_encode_tables(Context& c, const char* who);
// values: host [batch][N], every word < t (the caller has checked) -> out_dev [batch][rows][N] (batch stride sout, even; out_dev
// 16-byte aligned).  Queues on s and returns without waiting, but has finished reading `values`.  The one code path of
// lsa_bfv_encode and of the linear transform's diagonals.
void bfv_encode_rows(Context& c, int level, int form, const u64* values, u64* out_dev, long long sout, int batch, hipStream_t s);
// The encoder from the coefficient row on: coef [batch][N] on the device (batch stride scoef, 0: one row for the batch), words in
// [0, t), t below every modulus written (the caller has checked) -> form BFV_PT_MUL or BFV_PT_EXT in out_dev.  Queues on s, no
// host copy and no wait: the tail of bfv_encode_rows and the whole of lsa_bfv_plain_lift.
void bfv_lift_rows(Context& c, int level, int form, const u64* coef, long long scoef, u64* out_dev, long long sout, int batch,
                   hipStream_t s);
// the public entry point: every check of include/lattisense_amd.h, then bfv_encode_rows and a wait for s
void bfv_encode(Context& c, int level, int form, const u64* values, u64* out_dev, long long sout, int batch, hipStream_t s);

}  // namespace lsa
