// switches.h — every run-time (environment) switch of the library: one table, the only getenv of csrc/.
// Plain C++17 (task_graph.cpp and the host tests include it without HIP).  The compile-time switches are in build_flags.h.
//
// kind       how the value is parsed
//   OFF_IF_0       default on; off when the value starts with '0'
//   ON_IF_SET      default off; on when the variable exists, whatever it holds ("0" and "" included)
//   OVERRIDE_BOOL  unset: the default; else value[0] != '0'
//   INT            unset: the default; else atoi(value) & mask, at least lo
//   DOUBLE         unset: the default; else atof(value)
//   TRISTATE       unset: the default; "0..." = 0, "1..." = 1, anything else = 2
// lifetime   when the library asks (the call site decides; tests/test_switches_host.py keeps this column honest)
//   CALL     every call of the operator: may be flipped inside a process
//   PROCESS  once per process (cached in the accessor): only a fresh process sees another value
//   CONTEXT  when a context is created
//   PLAN     when a plan or a task is created (the description says which)
// A row is X(name, accessor, kind, lifetime, description, default...) -> sw::accessor(); an XD row takes the default from its
// caller, sw::accessor(dflt).  sw::accessor_of(value[, dflt]) is the uncached parse of a value.  INTEGRATION.md section 6
// shows this table.
#pragma once
#include <cstdlib>
#include <cstring>

#define LSA_SWITCHES(X, XD)                                                                                                        \
    X(LSA_NTT_R16, ntt_r16, OFF_IF_0, PROCESS,                                                                                     \
      "A/B: `=0` runs every transform pass on the staged kernel (`k_ntt_pass`) instead of the radix-16-squared passes "           \
      "(`k_ntt_r16`)", true)                                                                                                       \
    X(LSA_NTT_R8X3, ntt_r8x3, OFF_IF_0, PROCESS,                                                                                   \
      "A/B: `=0` runs the nine-stage second pass of N = 2^17 / 2^18 on the staged kernel instead of `k_ntt_r8x3`", true)           \
    X(LSA_R16_PRO, r16_pro, OFF_IF_0, PROCESS, "A/B: `=0` runs the fused-prologue first pass on the staged kernel", true)          \
    X(LSA_KS_FUSED, ks_fused, OFF_IF_0, CALL,                                                                                      \
      "A/B: `=0` runs the extension transform's second pass and the key MAC as separate kernels (a key uploaded under either "    \
      "setting works with both)", true)                                                                                            \
    X(LSA_KS_FUSED_ENGINES, ks_fused_engines, INT, PROCESS,                                                                        \
      "bit mask (two bits) of the butterfly engines whose target limbs take the fused key MAC: `3` fuses integer-engine limbs "   \
      "too (default 2: FP64-engine limbs only)", 2, 3)                                                                             \
    X(LSA_KSMAC_XCD, ksmac_xcd, OFF_IF_0, CALL,                                                                                    \
      "A/B: `=0` orders the fused kernel's workgroups plainly batch-fastest (default: the batch of one key tile is dealt to one " \
      "XCD)", true)                                                                                                                \
    X(LSA_ROT_SCATTER, rot_scatter, OFF_IF_0, CALL,                                                                                \
      "A/B: `=0` makes rotations write an intermediate and run a permutation kernel (default: the automorphism is applied by "    \
      "the store of the key switch's last pass / of the double-hoisted key MAC)", true)                                            \
    X(LSA_HMULT_FOLD, hmult_fold, OFF_IF_0, CALL,                                                                                  \
      "A/B: `=0` makes CKKS HMult+relin+rescale run `k_tensor`, then the key switch on its d2 and the merged tail with d0/d1 as " \
      "base (default with fused tails: d2 = a1*b1 formed by the key switch's inverse transform as it loads, and the tensor "      \
      "product folded into the key MAC)", true)                                                                                    \
    X(LSA_BFV_FOLD, bfv_fold, OFF_IF_0, CALL,                                                                                      \
      "A/B: `=0` runs BFV multiply with its copies and separate element-wise steps (default: folded into the transforms' source " \
      "and the conversions)", true)                                                                                                \
    X(LSA_PTMUL_FUSED, ptmul_fused, OFF_IF_0, CALL,                                                                                \
      "A/B and fallback: `=0` runs BFV ct x pt_mul as the forward transform, a Montgomery multiply(-accumulate) kernel "          \
      "(`k_mont_muladd`) and the inverse transform (default: the product is taken by the store of the forward transform's last "  \
      "pass)", true)                                                                                                               \
    X(LSA_ROTMAC_FUSED, rotmac_fused, OFF_IF_0, CALL,                                                                              \
      "A/B and fallback: `=0` makes each rotation term of `lsa_bfv_rotate_mac_plain_mul` run the NTT-domain ModDown into the "    \
      "workspace, then `k_mont_muladd` (default: the product and the running sum are taken by the ModDown's last store)", true)    \
    X(LSA_LT_BLOCKED_MAC, lt_blocked_mac, OFF_IF_0, CALL,                                                                          \
      "A/B and parity: `=0` makes a linear transform with more than 8 baby or 8 giant steps form its inner sums with one "        \
      "`k_mac_plain` launch per giant step and 16 terms (default: 8 x 8 blocks of `k_mac_plain_multi`, each adding to the sums "  \
      "the previous block left)", true)                                                                                            \
    X(LSA_LT_GIANT_SCATTER, lt_giant_scatter, OVERRIDE_BOOL, CALL,                                                                 \
      "A/B and parity: `=1` / `=0` sends the giant-step rotations of `lsa_ckks_linear_transform` through the accumulating "       \
      "scatter of the key MAC / through MAC + `k_permute_ext` (default 0, DESIGN 4.7; `LSA_ROT_SCATTER=0` forces the "            \
      "permutation form)", false)                                                                                                  \
    X(LSA_BT_NO_MULTI_MAC, bt_no_multi_mac, ON_IF_SET, CALL, "A/B: one plaintext-MAC launch per giant step", false)                \
    X(LSA_MACM_NO_XCD, macm_no_xcd, ON_IF_SET, CALL, "A/B: the multi-MAC's workgroups without the XCD deal", false)                \
    X(LSA_BT_STOP, bt_stop, INT, CALL,                                                                                             \
      "diagnostic: `=<step>` makes a bootstrap return the first out_level + 1 limbs of that step's intermediate (default -1: "    \
      "none)", -1)                                                                                                                 \
    X(LSA_TASK_TRACE, task_trace, ON_IF_SET, CALL, "per-level / per-chunk timings of a task run on stderr", false)                 \
    XD(LSA_STAGE_THREADS, stage_threads, INT, PROCESS,                                                                             \
       "host threads that stage task inputs and outputs, at least 1 and at most 32 (default: up to 14, by the machine's CPUs)",   \
       dflt, -1, 1)                                                                                                                \
    X(LSA_NTT_MU_A, ntt_mu_a, INT, CONTEXT,                                                                                        \
      "A/B: stages of the first pass of two-pass transforms (default 0: floor(log N / 2))", 0)                                     \
    XD(LSA_NTT_FP_RAW, ntt_fp_raw, OVERRIDE_BOOL, CONTEXT,                                                                         \
       "`=0`: FP64-engine limbs cross between the two NTT passes as canonical u64 instead of reduced doubles (default 1: "      \
       "doubles)", dflt)                                                                                                           \
    XD(LSA_NTT_WIDE, ntt_wide, TRISTATE, CONTEXT,                                                                                  \
       "N = 2^13 / 2^14 transforms: `=0` / `=1` never / always use the whole-limb single-pass plan (default: chosen per launch)", \
       dflt)                                                                                                                       \
    X(LSA_BC_NO_SPLIT, bc_no_split, ON_IF_SET, PLAN,                                                                               \
      "base conversion: 128-bit accumulate for every modulus size (default: 29-bit split columns below 2^58); read when a "       \
      "context makes the first base-conversion plan of a shape",                                                                   \
      false)                                                                                                                       \
    XD(LSA_BT_DOUBLE_HOIST, bt_double_hoist, OVERRIDE_BOOL, PLAN,                                                                  \
       "read when a bootstrap plan is made: `=0` makes baby-step / giant-step matrices divide by P once per rotation (default: "  \
       "double hoisting -- sums over Q u P, one division per giant step + one at the end; the plan's plaintexts then carry the "  \
       "special primes' rows)", dflt)                                                                                              \
    X(LSA_NO_GRAPH_FUSION, no_graph_fusion, ON_IF_SET, PLAN,                                                                       \
      "read when a task is created: run the graph exactly as compiled (no accumulation / mult->relin->rescale / rotate-and-MAC "  \
      "fusion)", false)                                                                                                            \
    X(LSA_NO_KEY_CACHE, no_key_cache, ON_IF_SET, PLAN,                                                                             \
      "read when a task is created: upload and convert every evaluation key on every run (reference behaviour)", false)            \
    X(LSA_NO_PIPELINE, no_pipeline, ON_IF_SET, PLAN,                                                                               \
      "read when a task is created, and again by a run on another number of devices: one lane, levels run strictly in order "     \
      "(no H2D / compute / D2H overlap across subgraphs)", false)                                                                  \
    X(LSA_PIPELINE_MIN_MIB, pipeline_min_mib, DOUBLE, PLAN,                                                                        \
      "read with `LSA_NO_PIPELINE`: input volume in MiB from which independent subgraphs are pipelined (default 256)", 256.0)      \
    X(LSA_POOL_MAX_DEV_GIB, pool_max_dev_gib, DOUBLE, PLAN,                                                                        \
      "read when a task is created: cap in GiB on the device bytes it keeps pooled per (device, lane) (default 48)", 48.0)         \
    X(LSA_POOL_MAX_PIN_GIB, pool_max_pin_gib, DOUBLE, PLAN,                                                                        \
      "read when a task is created: cap in GiB on the pinned bytes it keeps pooled per device (default 16)", 16.0)

namespace lsa {
namespace sw {

inline bool parse_OFF_IF_0(const char* v, bool) { return !(v && v[0] == '0'); }
inline bool parse_ON_IF_SET(const char* v, bool) { return v != nullptr; }
inline bool parse_OVERRIDE_BOOL(const char* v, bool dflt) { return v ? v[0] != '0' : dflt; }
inline int parse_INT(const char* v, int dflt, int mask = -1, int lo = -2147483647 - 1) {
    if (!v) return dflt;
    const int x = std::atoi(v) & mask;
    return x < lo ? lo : x;
}
inline double parse_DOUBLE(const char* v, double dflt) { return v ? std::atof(v) : dflt; }
inline int parse_TRISTATE(const char* v, int dflt) { return !v ? dflt : v[0] == '0' ? 0 : v[0] == '1' ? 1 : 2; }
using OVERRIDE_BOOL_t = bool;
using INT_t = int;
using TRISTATE_t = int;

#define LSA_SW_READ_CALL(expr) return expr;
#define LSA_SW_READ_CONTEXT(expr) return expr;
#define LSA_SW_READ_PLAN(expr) return expr;
#define LSA_SW_READ_PROCESS(expr) \
    static const auto cached = expr; \
    return cached;
#define LSA_SW_X(NAME, fn, KIND, LIFE, DESC, ...)                                  \
    inline auto fn##_of(const char* v) { return parse_##KIND(v, __VA_ARGS__); }   \
    inline auto fn() { LSA_SW_READ_##LIFE(fn##_of(std::getenv(#NAME))) }
#define LSA_SW_XD(NAME, fn, KIND, LIFE, DESC, ...)                                                 \
    inline auto fn##_of(const char* v, KIND##_t dflt) { return parse_##KIND(v, __VA_ARGS__); }     \
    inline auto fn(KIND##_t dflt) { LSA_SW_READ_##LIFE(fn##_of(std::getenv(#NAME), dflt)) }
LSA_SWITCHES(LSA_SW_X, LSA_SW_XD)
#undef LSA_SW_X
#undef LSA_SW_XD

struct Row {
    const char *name, *kind, *lifetime, *text;
};
#define LSA_SW_ROW(NAME, fn, KIND, LIFE, DESC, ...) {#NAME, #KIND, #LIFE, DESC},
inline constexpr Row table[] = {LSA_SWITCHES(LSA_SW_ROW, LSA_SW_ROW)};
#undef LSA_SW_ROW

}  // namespace sw
}  // namespace lsa
