// task_dispatch.hip — from the backend nodes of a task graph to launches of the operator layer: drop-in for
// mega_ag_executors_gpu.cu (bind_gpu_executor and the per-op executors), re-designed for MI355X:
//
//   * LEVEL-BATCHED dispatch: nodes of one topological level that perform the same operator on the same shapes (the frontend
//     emits n_op identical disjoint subgraphs, e.g. examples/benchmark_gpu/benchmark_gpu.py:29-33) are executed as ONE batched
//     launch sequence of the operator layer.  A 1024-op task becomes a handful of large launches that fill 256 CUs, not 7k
//     tiny ones.
//   * device data of a batch lives in one slab with a fixed stride, so operands of the next level are usually already
//     contiguous; otherwise they are gathered with device-to-device copies.
#include <unordered_set>

#include "task_internal.h"

using namespace lsa;
using namespace lsa::task;

namespace {

const char* op_name(OperationType op) {
    switch (op) {
        case OperationType::ADD: return "add";
        case OperationType::SUB: return "sub";
        case OperationType::NEGATE: return "neg";
        case OperationType::MULTIPLY: return "mult";
        case OperationType::RELINEARIZE: return "relin";
        case OperationType::RESCALE: return "rescale";
        case OperationType::DROP_LEVEL: return "drop_level";
        case OperationType::ROTATE_COL: return "rotate_col";
        case OperationType::ROTATE_ROW: return "rotate_row";
        case OperationType::MAC_WO_PARTIAL_SUM: return "cmp_sum";
        case OperationType::MAC_W_PARTIAL_SUM: return "cmpac_sum";
        case OperationType::BOOTSTRAP: return "bootstrap";
        case OperationType::FUSED_MULT_RELIN_RESCALE: return "mult+relin+rescale";
        case OperationType::FUSED_ROTATE_MAC: return "rotate+cmp_sum";
        default: return "?";
    }
}

}  // namespace

// The operator surface of mega_ag_runners/mega_ag_executors.h:53-54: validates that this backend implements the node
// (the reference throws at bind time for unsupported combinations, mega_ag_executors_gpu.cu:212,481,498).  Backend nodes
// are dispatched in batches by Dispatcher::run_gpu_bucket; this records nothing but the verdict.
void bind_gpu_executor(ComputeNode& node, Algo algorithm) {
    if (!node.fhe_prop) throw std::runtime_error("FHE property not found for compute node");
    const OperationType op = node.op();
    auto unsupported = [&](const std::string& why) {
        throw std::runtime_error(std::string("Unsupported operation type for GPU ") + (algorithm == ALGO_BFV ? "BFV" : "CKKS") +
                                 ": " + op_name(op) + " (" + why + ")");
    };
    for (auto* in : node.input_nodes)
        if (!in->fhe_prop) throw std::runtime_error("FHE property not found for input node " + std::to_string(in->index));
    switch (op) {
        case OperationType::ADD:
        case OperationType::SUB: break;   // ct+-ct, ct+-pt, ct+-ring-t pt
        case OperationType::MULTIPLY:
            if (node.input_nodes.size() == 2 && algorithm == ALGO_BFV) {
                // BFV ct x pt_mul, the plaintext on either side (the reference's find_plaintext_node), at the ciphertext's level
                const DatumNode *x = node.input_nodes[0], *y = node.input_nodes[1];
                const DatumNode* pt = is_ptmul_node(y) && !is_plain_node(x) ? y : is_ptmul_node(x) && !is_plain_node(y) ? x : nullptr;
                if (pt) {
                    const DatumNode* ct = pt == y ? x : y;
                    if (pt->fhe_prop->level != ct->fhe_prop->level)
                        unsupported("pt_mul plaintext at level " + std::to_string(pt->fhe_prop->level) + ", the ciphertext at " +
                                    std::to_string(ct->fhe_prop->level));
                    break;
                }
            }
            if (node.input_nodes.size() == 2 && is_plain_node(node.input_nodes[1]) && !is_ringt_node(node.input_nodes[1]) &&
                algorithm == ALGO_BFV)
                throw std::runtime_error("Multiply with plaintext only supported for CKKS scheme");  // executors_gpu.cu:212
            if (node.input_nodes.size() == 2 && is_plain_node(node.input_nodes[0]))
                unsupported("plaintext as the first operand (BFV pt_mul only)");
            break;
        case OperationType::NEGATE:
        case OperationType::RELINEARIZE:
        case OperationType::RESCALE:
        case OperationType::ROTATE_ROW:
        case OperationType::FUSED_MULT_RELIN_RESCALE:
            break;
        case OperationType::FUSED_ROTATE_MAC:   // made by TaskGraph::fuse_rotate_mac, BFV only
            if (algorithm != ALGO_BFV) unsupported("BFV only");
            if (!node.fhe_prop->p || node.fhe_prop->p->sum_cnt < 1) throw std::runtime_error("Sum count not found in FHE property");
            break;
        case OperationType::ROTATE_COL:
            if (!node.fhe_prop->p) throw std::runtime_error("Rotation step not found in FHE property");
            break;
        case OperationType::DROP_LEVEL:
            if (algorithm == ALGO_BFV) throw std::runtime_error("DROP_LEVEL only supported for CKKS scheme");
            break;
        case OperationType::MAC_WO_PARTIAL_SUM:
        case OperationType::MAC_W_PARTIAL_SUM: {
            if (!node.fhe_prop->p) throw std::runtime_error("Sum count not found in FHE property");
            const int n = node.fhe_prop->p->sum_cnt;
            const size_t pt0 = (size_t)n + (op == OperationType::MAC_W_PARTIAL_SUM ? 1 : 0);
            if (node.input_nodes.size() != pt0 + (size_t)n) unsupported("compressed plaintext blocks");
            if (algorithm == ALGO_BFV) {   // pt_mul terms: all of them, at the ciphertexts' level
                int ptmul = 0;
                for (int i = 0; i < n; i++) ptmul += is_ptmul_node(node.input_nodes[pt0 + i]) ? 1 : 0;
                if (ptmul > 0 && ptmul < n) unsupported("pt_mul and other plaintext flavours in one multiply-accumulate");
                if (ptmul == n) {
                    for (int i = 0; i < n; i++)
                        if (node.input_nodes[pt0 + i]->fhe_prop->level != node.input_nodes[0]->fhe_prop->level)
                            unsupported("pt_mul plaintext at level " + std::to_string(node.input_nodes[pt0 + i]->fhe_prop->level) +
                                        ", the ciphertexts at " + std::to_string(node.input_nodes[0]->fhe_prop->level));
                    break;
                }
            }
            if (algorithm == ALGO_BFV && !is_ringt_node(node.input_nodes[pt0]))
                throw std::runtime_error("Multiply with plaintext only supported for CKKS scheme");  // executors_gpu.cu:349,405
            break;
        }
        case OperationType::BOOTSTRAP:   // inputs [ct, rlk, glk..., swk_dts, swk_std] (frontend/custom_task.py:1952-2002)
            if (algorithm != ALGO_CKKS) throw std::runtime_error("BOOTSTRAP only supported for CKKS scheme");  // executors_gpu.cu:424
            if (node.input_nodes.size() < 5) unsupported("bootstrap node without its keys");
            break;
        default: unsupported("unknown");
    }
}

namespace lsa {
namespace task {

// bootstrapping plan from the task's `parameter` block (reference: gpu_wrapper.cu:86-117)
Bootstrap& Dispatcher::bootstrap_plan(Lane& ln) {
    Context& c = ln.c;
    std::lock_guard<std::mutex> lk(bootstrap_mu);
    auto it = bootstrap_plans.find(&c);
    if (it != bootstrap_plans.end()) return *it->second;
    const mjson::Value& P = g.parameter;
    LSA_REQUIRE(P.contains("btp_output_level"), "bootstrap node in a task without bootstrapping parameters");
    // (the sine TYPE is not among the fields the reference forwards to its GPU library, gpu_wrapper.cu:94-103; Cos1 is what the
    // frontend's parameter sets say and what is implemented)
    LSA_REQUIRE(!P.contains("btp_eval_mod_sine_type") || P["btp_eval_mod_sine_type"].as_string() == "Cos1",
                "bootstrap: only the Cos1 sine type is implemented");
    const int sine_deg = (int)P["btp_eval_mod_sine_deg"].as_int(), arcsine_deg = (int)P["btp_eval_mod_arcsine_deg"].as_int();
    int log_slots = 0;
    if (P.contains("slots")) {
        const long long slots = P["slots"].as_int();
        LSA_REQUIRE(slots >= 2 && slots <= c.n / 2 && (slots & (slots - 1)) == 0, "bootstrap: slot count must be a power of two <= N/2");
        while ((1LL << log_slots) < slots) log_slots++;
    }
    LSA_REQUIRE(sine_deg >= 1 && sine_deg <= 63, "bootstrap: sine degree outside 1..63");
    LSA_REQUIRE(arcsine_deg >= 0 && arcsine_deg <= 15 && (arcsine_deg == 0 || (arcsine_deg & 1)), "bootstrap: arcsine degree must be 0 or odd and at most 15");
    const int cts_depth = (int)P["btp_cts_depth"].as_int(), stc_depth = (int)P["btp_stc_depth"].as_int();
    LSA_REQUIRE(P["btp_cts_start_level"].as_int() == c.nq - 1 && P["btp_eval_mod_start_level"].as_int() == c.nq - 1 - cts_depth,
                "bootstrap: level plan differs from the one implemented");
    const double scale = P["scale"].as_double();
    Bootstrap* b = bootstrap_create(c, cts_depth, stc_depth, (int)P["btp_eval_mod_k"].as_int(),
                                    (int)P["btp_eval_mod_double_angle"].as_int(), P["btp_eval_mod_message_ratio"].as_double(),
                                    scale, scale, log_slots, ln.s, sine_deg, arcsine_deg);
    LSA_REQUIRE(bootstrap_out_level(*b) == P["btp_output_level"].as_int() &&
                    P["btp_stc_start_level"].as_int() == bootstrap_out_level(*b) + stc_depth,
                "bootstrap: level plan differs from the one implemented");
    bootstrap_plans[&c].reset(b);
    return *b;
}

// operand `pos` of every node of the bucket as (base, stride); gathers with D2D copies if not already strided
Dispatcher::Operand Dispatcher::gather(Lane& ln, const std::vector<ComputeNode*>& nodes, int pos, Avail& avail, size_t words) {
    std::vector<DatumP> d;
    for (auto* n : nodes) d.push_back(std::any_cast<DatumP>(avail.at(n->input_nodes[pos]->index)));
    Operand o{d[0]->ptr, (long long)words, nullptr};
    if (d.size() == 1) return o;
    const long long st = d[1]->ptr - d[0]->ptr;
    bool strided = st >= (long long)words || st == 0;
    for (size_t i = 1; i < d.size() && strided; i++) strided = (d[i]->ptr - d[0]->ptr) == st * (long long)i;
    if (strided && st != 0) {
        o.stride = st;
        return o;
    }
    o.keep = ln.dslab(words * d.size());
    for (size_t i = 0; i < d.size(); i++)
        LSA_HIP(hipMemcpyAsync(o.keep->ptr + words * i, d[i]->ptr, words * sizeof(u64), hipMemcpyDeviceToDevice, ln.s));
    o.ptr = o.keep->ptr;
    o.stride = (long long)words;
    ln.defer(o.keep);
    return o;
}

std::string Dispatcher::signature(const ComputeNode* n) const {
    std::string sg = std::to_string((int)n->op());
    if (n->op() == OperationType::FUSED_ROTATE_MAC) {   // only nodes with the same term plan batch together
        const RotMacPlan& pl = g.rotmac_plans.at(n->index);
        sg += pl.partial ? "p" : "-";
        for (size_t i = 0; i < pl.key_pos.size(); i++) sg += "," + std::to_string(pl.key_pos[i]) + (pl.row[i] ? "r" : "");
    }
    for (auto* in : n->input_nodes) {
        sg += "|" + std::to_string((int)in->datum_type) + ":" + std::to_string(in->fhe_prop->level) + ":" +
              std::to_string(in->fhe_prop->degree);
        // pt, pt_mul and pt_ringt all arrive as TYPE_PLAINTEXT: the plaintext's treatment (lift, transform) is decided per
        // bucket from its first node, so the flavour is part of the signature
        if (in->datum_type == TYPE_PLAINTEXT) {
            sg += (in->fhe_prop->p && in->fhe_prop->p->is_ringt) ? "r" : (in->fhe_prop->is_ntt ? "n" : "c");
            if (in->fhe_prop->is_mform) sg += "m";
        }
        // all nodes of a bucket must use the SAME key datum
        if (in->datum_type != TYPE_CIPHERTEXT && in->datum_type != TYPE_PLAINTEXT) sg += "#" + std::to_string(in->index);
    }
    sg += ">" + std::to_string(n->output_nodes[0]->fhe_prop->level) + ":" + std::to_string(n->input_nodes.size());
    return sg;
}

void Dispatcher::run_gpu_bucket(Lane& ln, const std::vector<ComputeNode*>& nodes, Avail& avail) {
    Context& c = ln.c;
    const hipStream_t s = ln.s;
    const long long N = c.n;
    const ComputeNode* n0 = nodes[0];
    const OperationType op = n0->op();
    const int m = (int)nodes.size();
    // BFV ct x pt_mul may name the plaintext first (bind_gpu_executor): the ciphertext sets the shapes
    const bool ptmul_first = g.algo == ALGO_BFV && op == OperationType::MULTIPLY && n0->input_nodes.size() == 2 &&
                             is_ptmul_node(n0->input_nodes[0]);
    const DatumNode* in0 = n0->input_nodes[ptmul_first ? 1 : 0];
    const int lvl = in0->fhe_prop->level, L = lvl + 1;
    const int polys_in = in0->fhe_prop->degree + 1;
    const int out_lvl = n0->output_nodes[0]->fhe_prop->level;
    const bool bfv = g.algo == ALGO_BFV;
    const size_t w_in = (size_t)polys_in * L * N;
    int out_polys = polys_in;
    if (op == OperationType::MULTIPLY && !(n0->input_nodes.size() == 2 && (is_plain_node(n0->input_nodes[1]) || ptmul_first)))
        out_polys = 3;
    if (op == OperationType::RELINEARIZE || op == OperationType::FUSED_MULT_RELIN_RESCALE || op == OperationType::FUSED_ROTATE_MAC)
        out_polys = 2;
    const size_t w_out = (size_t)out_polys * (out_lvl + 1) * N;
    auto out_slab = ln.dslab(w_out * m);
    u64* out = out_slab->ptr;
    const long long so = (long long)w_out;
    Operand a = gather(ln, nodes, ptmul_first ? 1 : 0, avail, w_in);
    RowMap rmL;
    rmL.period = L;
    for (int i = 0; i < L; i++) rmL.mod_of[i] = (unsigned char)i;

    auto key_of = [&](int pos) -> const Key& { return std::any_cast<KeyP>(avail.at(n0->input_nodes[pos]->index))->key; };
    // plaintext operand `pos` of every node as [m][L][N] limbs in the domain the operator needs.
    //   full plaintext: used as loaded (CKKS: NTT domain; BFV: coefficient domain, already scaled)
    //   ring-t plaintext (one limb): lifted per `ringt_mode` (kernels.hip k_lift_ringt), then NTT'd if `to_ntt`
    auto plain_operand = [&](int pos, int ringt_mode, bool to_ntt) -> Operand {
        if (!is_ringt_node(n0->input_nodes[pos])) return gather(ln, nodes, pos, avail, (size_t)L * N);
        Operand raw = gather(ln, nodes, pos, avail, (size_t)N);
        Operand o{nullptr, (long long)L * N, ln.dslab((size_t)m * L * N)};
        ln.defer(o.keep);
        launch_lift_ringt(c, ringt_mode, lvl, raw.ptr, raw.stride, o.keep->ptr, o.stride, m, s);
        if (to_ntt) launch_ntt(c, o.keep->ptr, o.keep->ptr, m, o.stride, L, rmL, false, s);
        o.ptr = o.keep->ptr;
        return o;
    };

    switch (op) {
        case OperationType::ADD:
        case OperationType::SUB: {
            const EwOp ew = op == OperationType::ADD ? EW_ADD : EW_SUB;
            if (n0->input_nodes.size() == 1) {
                launch_elementwise(c, ew, a.ptr, a.ptr, out, m, a.stride, a.stride, so, polys_in * L, rmL, s);
            } else if (bfv && is_plain_node(n0->input_nodes[1]) && is_ringt_node(n0->input_nodes[1]) && polys_in >= 2 && polys_in <= 3) {
                // BFV ct +- ring-t pt in one launch: the plaintext is scaled up by Q/t with rounding as c0 is read, the other
                // polynomials are copied by the same lanes (bfv_plain.hip; the words of lift mode 2 + copy + add)
                Operand b = gather(ln, nodes, 1, avail, (size_t)N);
                launch_bfv_addsub_plain(c, ew == EW_ADD ? 0 : 1, lvl, polys_in, a.ptr, a.stride, b.ptr, b.stride, out, so, m, s);
            } else if (is_plain_node(n0->input_nodes[1])) {
                // CKKS: plaintext limbs in the NTT domain (ring-t: centred lift + NTT); BFV: coefficient domain, a full
                // plaintext already scaled
                Operand b = plain_operand(1, bfv ? 2 : 0, !bfv);
                std::vector<int> rows(polys_in * L);
                for (size_t i = 0; i < rows.size(); i++) rows[i] = (int)i;
                launch_copy_rows(c, a.ptr, a.stride, out, so, polys_in * L, rows.data(), m, s);
                launch_elementwise(c, ew, a.ptr, b.ptr, out, m, a.stride, b.stride, so, L, rmL, s);  // c0 +/- pt
            } else {
                Operand b = gather(ln, nodes, 1, avail, w_in);
                launch_elementwise(c, ew, a.ptr, b.ptr, out, m, a.stride, b.stride, so, polys_in * L, rmL, s);
            }
            break;
        }
        case OperationType::NEGATE:
            launch_elementwise(c, EW_NEG, a.ptr, nullptr, out, m, a.stride, 0, so, polys_in * L, rmL, s);
            break;
        case OperationType::MULTIPLY: {
            if (bfv && n0->input_nodes.size() == 2 && (ptmul_first || is_ptmul_node(n0->input_nodes[1]))) {   // ct x pt_mul
                Operand b = gather(ln, nodes, ptmul_first ? 0 : 1, avail, (size_t)L * N);
                bfv_mult_plain_mul(c, lvl, a.ptr, b.ptr, out, m, a.stride, b.stride, so, s);
                break;
            }
            if (n0->input_nodes.size() == 2 && is_plain_node(n0->input_nodes[1])) {
                if (!bfv) {  // CKKS ct * pt, both NTT domain (ring-t: centred lift + NTT first)
                    Operand b = plain_operand(1, 0, true);
                    for (int p = 0; p < polys_in; p++)
                        launch_elementwise(c, EW_MUL, a.ptr + (size_t)p * L * N, b.ptr, out + (size_t)p * L * N, m,
                                           a.stride, b.stride, so, L, rmL, s);
                } else {     // BFV ct * ring-t pt: NTT(ct) . NTT(pt as residues), back to coefficients
                    Operand b = plain_operand(1, 1, true);
                    std::vector<int> rows(polys_in * L);
                    for (size_t i = 0; i < rows.size(); i++) rows[i] = (int)i;
                    launch_copy_rows(c, a.ptr, a.stride, out, so, polys_in * L, rows.data(), m, s);
                    launch_ntt(c, out, out, m, so, polys_in * L, rmL, false, s);
                    for (int p = 0; p < polys_in; p++)
                        launch_elementwise(c, EW_MUL, out + (size_t)p * L * N, b.ptr, out + (size_t)p * L * N, m, so,
                                           b.stride, so, L, rmL, s);
                    launch_ntt(c, out, out, m, so, polys_in * L, rmL, true, s);
                }
                break;
            }
            Operand b = n0->input_nodes.size() == 1 ? a : gather(ln, nodes, 1, avail, w_in);
            LSA_REQUIRE(polys_in == 2, "ciphertext multiply expects degree-1 operands");
            if (bfv) bfv_mult(c, lvl, a.ptr, b.ptr, out, m, a.stride, b.stride, so, s);
            else launch_tensor(c, a.ptr, b.ptr, out, m, a.stride, b.stride, so, L, rmL, s);
            break;
        }
        case OperationType::FUSED_MULT_RELIN_RESCALE: {   // inputs [a, (b,) rlk]
            LSA_REQUIRE(!bfv && polys_in == 2 && out_lvl == lvl - 1, "fused mult+relin+rescale: unexpected shape");
            const int kpos = (int)n0->input_nodes.size() - 1;
            Operand b = kpos == 1 ? a : gather(ln, nodes, 1, avail, w_in);
            ckks_mult_relin_rescale(c, lvl, a.ptr, b.ptr, key_of(kpos), out, m, a.stride, b.stride, so, s);
            break;
        }
        case OperationType::BOOTSTRAP: {
            LSA_REQUIRE(!bfv && polys_in == 2 && lvl == 0, "bootstrap expects a degree-1 CKKS ciphertext at level 0");
            Bootstrap& plan = bootstrap_plan(ln);
            LSA_REQUIRE(out_lvl == bootstrap_out_level(plan), "bootstrap: output datum is not at the bootstrap output level");
            GaloisKeys glk;
            std::vector<const Key*> swk;
            for (size_t i = 2; i < n0->input_nodes.size(); i++) {
                const DatumNode* kd = n0->input_nodes[i];
                if (kd->datum_type == TYPE_GALOIS_KEY) {
                    LSA_REQUIRE(kd->fhe_prop && kd->fhe_prop->p, "Galois element missing on the key datum");
                    glk.insert(kd->fhe_prop->p->galois_element, &key_of((int)i));
                } else if (kd->datum_type == TYPE_SWITCH_KEY) {
                    swk.push_back(&key_of((int)i));
                }
            }
            LSA_REQUIRE(swk.empty() || swk.size() == 2, "bootstrap: swk_dts and swk_std come as a pair");
            bootstrap_run(plan, a.ptr, a.stride, out, so, m, key_of(1), glk, swk.empty() ? nullptr : swk[0],
                          swk.empty() ? nullptr : swk[1], s);
            break;
        }
        case OperationType::RELINEARIZE:
            LSA_REQUIRE(polys_in == 3, "relinearize expects a degree-2 ciphertext");
            if (bfv) bfv_relin(c, lvl, a.ptr, key_of(1), out, m, a.stride, so, s);
            else ckks_relin(c, lvl, a.ptr, key_of(1), out, m, a.stride, so, s);
            break;
        case OperationType::RESCALE:
            LSA_REQUIRE(out_lvl == lvl - 1, "rescale must drop exactly one level");
            if (bfv) bfv_rescale(c, lvl, polys_in, a.ptr, out, m, a.stride, so, s);
            else ckks_rescale(c, lvl, polys_in, a.ptr, out, m, a.stride, so, s);
            break;
        case OperationType::DROP_LEVEL: {
            LSA_REQUIRE(out_lvl < lvl && out_lvl >= 0, "drop_level must lower the level");
            std::vector<int> rows;
            for (int p = 0; p < polys_in; p++)
                for (int i = 0; i <= out_lvl; i++) rows.push_back(p * L + i);
            launch_copy_rows(c, a.ptr, a.stride, out, so, (int)rows.size(), rows.data(), m, s);
            break;
        }
        case OperationType::ROTATE_COL:
        case OperationType::ROTATE_ROW: {
            LSA_REQUIRE(polys_in == 2, "rotation expects a degree-1 ciphertext");
            const DatumNode* kd = n0->input_nodes[1];
            u64 gel = op == OperationType::ROTATE_ROW ? 2 * (u64)c.n - 1 : (kd->fhe_prop->p ? kd->fhe_prop->p->galois_element : 0);
            LSA_REQUIRE(gel != 0, "Galois element missing on the key datum");
            if (bfv) bfv_rotate(c, lvl, a.ptr, gel, key_of(1), out, m, a.stride, so, s);
            else ckks_rotate(c, lvl, a.ptr, gel, key_of(1), out, m, a.stride, so, s);
            break;
        }
        case OperationType::FUSED_ROTATE_MAC: {   // inputs [X, (partial,) keys..., pts...], TaskGraph::rotmac_plans
            LSA_REQUIRE(bfv && polys_in == 2, "rotate-and-MAC expects a BFV degree-1 ciphertext");
            const RotMacPlan& pl = g.rotmac_plans.at(n0->index);
            const int n = (int)pl.key_pos.size();
            int nkeys = 0;
            for (int kp : pl.key_pos) nkeys += kp >= 0 ? 1 : 0;
            const int pt0 = 1 + (pl.partial ? 1 : 0) + nkeys;
            LSA_REQUIRE((int)n0->input_nodes.size() == pt0 + n, "rotate-and-MAC node: unexpected number of inputs");
            std::vector<u64> els(n);
            std::vector<const Key*> keys(n, nullptr);
            std::vector<const u64*> pp(n);
            std::vector<long long> ps_(n);
            for (int i = 0; i < n; i++) {
                els[i] = 1;
                if (pl.key_pos[i] >= 0) {
                    const DatumNode* kd = n0->input_nodes[pl.key_pos[i]];
                    els[i] = pl.row[i] ? 2 * (u64)c.n - 1 : (kd->fhe_prop->p ? kd->fhe_prop->p->galois_element : 0);
                    LSA_REQUIRE(els[i] != 0, "Galois element missing on the key datum");
                    keys[i] = &key_of(pl.key_pos[i]);
                }
                Operand pi = gather(ln, nodes, pt0 + i, avail, (size_t)L * N);
                pp[i] = pi.ptr;
                ps_[i] = pi.stride;
            }
            Operand part{nullptr, 0, nullptr};
            if (pl.partial) part = gather(ln, nodes, 1, avail, w_in);
            bfv_rotate_mac_plain_mul(c, lvl, a.ptr, n, els.data(), keys.data(), pp.data(), ps_.data(), part.ptr, part.stride, out,
                                     m, a.stride, so, s);
            break;
        }
        case OperationType::MAC_WO_PARTIAL_SUM:
        case OperationType::MAC_W_PARTIAL_SUM: {
            // inputs: ct_0..ct_{n-1}, (ct_partial,) pt_0..pt_{n-1}   (frontend/custom_task.py:1753-1836)
            // out = sum_i ct_i * pt_i (+ ct_partial); mega_ag_executors_gpu.cu:294-408 does multiply_plain + add_inplace
            const int n = n0->fhe_prop->p->sum_cnt;
            const bool with_partial = op == OperationType::MAC_W_PARTIAL_SUM;
            const int pt0 = n + (with_partial ? 1 : 0);
            LSA_REQUIRE((int)n0->input_nodes.size() == pt0 + n, "MAC node: unexpected number of inputs");
            const int rows = polys_in * L;
            if (!bfv) {   // CKKS: every operand is in the NTT domain already -> groups of <= 16 terms per launch
                Operand part{nullptr, 0, nullptr};
                if (with_partial) part = gather(ln, nodes, n, avail, w_in);
                for (int i0 = 0; i0 < n; i0 += LSA_MAC_MAX_TERMS) {
                    const int cnt = std::min(LSA_MAC_MAX_TERMS, n - i0);
                    const u64* cp[LSA_MAC_MAX_TERMS];
                    const u64* pp[LSA_MAC_MAX_TERMS];
                    long long cs_[LSA_MAC_MAX_TERMS], ps_[LSA_MAC_MAX_TERMS];
                    for (int i = 0; i < cnt; i++) {
                        Operand ci = i0 + i == 0 ? a : gather(ln, nodes, i0 + i, avail, w_in);
                        Operand pi = plain_operand(pt0 + i0 + i, 0, true);
                        cp[i] = ci.ptr;
                        cs_[i] = ci.stride;
                        pp[i] = pi.ptr;
                        ps_[i] = pi.stride;
                    }
                    // the first group adds the node's partial sum, later groups continue from `out`
                    const u64* acc = i0 == 0 ? part.ptr : out;
                    launch_mac_plain(c, cnt, cp, cs_, pp, ps_, acc, i0 == 0 ? part.stride : so, out, so, m, polys_in, L, rmL, s);
                }
                break;
            }
            if (is_ptmul_node(n0->input_nodes[pt0])) {   // BFV pt_mul terms (bind_gpu_executor: all of them)
                std::vector<const u64*> cp(n), pp(n);
                std::vector<long long> cs_(n), ps_(n);
                for (int i = 0; i < n; i++) {
                    Operand ci = i == 0 ? a : gather(ln, nodes, i, avail, w_in);
                    Operand pi = gather(ln, nodes, pt0 + i, avail, (size_t)L * N);
                    cp[i] = ci.ptr;
                    cs_[i] = ci.stride;
                    pp[i] = pi.ptr;
                    ps_[i] = pi.stride;
                }
                Operand part{nullptr, 0, nullptr};
                if (with_partial) part = gather(ln, nodes, n, avail, w_in);
                bfv_mac_plain_mul(c, lvl, n, cp.data(), cs_.data(), pp.data(), ps_.data(), part.ptr, part.stride, out, m, so, s);
                break;
            }
            u64* tmp = ln.temp((size_t)m * w_in);
            std::vector<int> all(rows);
            for (int i = 0; i < rows; i++) all[i] = i;
            for (int i = 0; i < n; i++) {
                Operand ci = i == 0 ? a : gather(ln, nodes, i, avail, w_in);
                Operand pi = plain_operand(pt0 + i, bfv ? 1 : 0, true);
                const u64* cptr = ci.ptr;
                long long cstride = ci.stride;
                if (bfv) {  // accumulate in the NTT domain, one inverse transform at the end (linear => identical residues)
                    launch_copy_rows(c, ci.ptr, ci.stride, tmp, (long long)w_in, rows, all.data(), m, s);
                    launch_ntt(c, tmp, tmp, m, (long long)w_in, rows, rmL, false, s);
                    cptr = tmp;
                    cstride = (long long)w_in;
                }
                for (int p = 0; p < polys_in; p++)
                    launch_muladd(c, EW_MUL, cptr + (size_t)p * L * N, pi.ptr, i == 0 ? nullptr : out + (size_t)p * L * N, so,
                                  out + (size_t)p * L * N, m, cstride, pi.stride, so, L, rmL, s);
            }
            if (bfv) launch_ntt(c, out, out, m, so, rows, rmL, true, s);
            if (with_partial) {
                Operand part = gather(ln, nodes, n, avail, w_in);
                launch_elementwise(c, EW_ADD, out, part.ptr, out, m, so, part.stride, so, rows, rmL, s);
            }
            break;
        }
        default: throw Error(LSA_ERR_ARG, std::string("operation not implemented on this backend: ") + op_name(op));
    }
    publish(avail, out_slab, (size_t)m, DevDatum{nullptr, nullptr, out_polys, out_lvl, false}, N, [&](size_t i) { return nodes[i]; });
    ln.defer(out_slab);  // (cheap: shared) keeps frees off the critical path until the level ends
}

// Buckets of one level.  Rotations of the SAME ciphertexts by different Galois elements (the frontend's rotate_cols /
// advanced_rotate_cols emit them: examples/benchmark_convolution, BFV_4_advanced_rotate_col) are hoisted: one
// decomposition of the inputs, then only the key MAC + ModDown + permutation per element (ckks_rotate_many /
// bfv_rotate_many; same residues as separate rotations).
void Dispatcher::run_buckets(Lane& ln, Split& sp, Avail& avail) {
    Context& c = ln.c;
    const hipStream_t s = ln.s;
    auto& buckets = sp.buckets;
    const std::vector<std::string>& order = sp.bucket_order;
    std::map<std::vector<NodeIndex>, std::vector<const std::string*>> rot_groups;
    const bool hoist = g.algo == ALGO_CKKS || g.algo == ALGO_BFV;
    if (hoist)
        for (auto& sg : order) {
            auto& nodes = buckets[sg];
            const OperationType op = nodes[0]->op();
            if (op != OperationType::ROTATE_COL && op != OperationType::ROTATE_ROW) continue;
            std::vector<NodeIndex> ins;
            for (auto* n : nodes) ins.push_back(n->input_nodes[0]->index);
            rot_groups[ins].push_back(&sg);
        }
    std::unordered_set<const std::string*> done;
    for (auto& sg : order) {
        if (done.count(&sg)) continue;
        auto& nodes = buckets[sg];
        const OperationType op = nodes[0]->op();
        std::vector<const std::string*>* group = nullptr;
        if (hoist && (op == OperationType::ROTATE_COL || op == OperationType::ROTATE_ROW)) {
            std::vector<NodeIndex> ins;
            for (auto* n : nodes) ins.push_back(n->input_nodes[0]->index);
            auto& gr = rot_groups[ins];
            if (gr.size() >= 2) group = &gr;
        }
        if (!group) {
            run_gpu_bucket(ln, nodes, avail);
            gpu_nodes += (int)nodes.size();
            gpu_batches++;
            continue;
        }
        // hoisted group: same inputs, one Galois element per member bucket
        const long long N = c.n;
        const ComputeNode* n0 = nodes[0];
        const int lvl = n0->input_nodes[0]->fhe_prop->level, L = lvl + 1, m = (int)nodes.size();
        LSA_REQUIRE(n0->input_nodes[0]->fhe_prop->degree == 1, "rotation expects a degree-1 ciphertext");
        const size_t w = (size_t)2 * L * N;
        Operand a = gather(ln, nodes, 0, avail, w);
        std::vector<u64> els;
        std::vector<const Key*> keys;
        std::vector<u64*> outs;
        std::vector<std::shared_ptr<Slab>> slabs;
        for (const std::string* member : *group) {
            auto& mn = buckets[*member];
            const ComputeNode* r0 = mn[0];
            const DatumNode* kd = r0->input_nodes[1];
            const u64 gel = r0->op() == OperationType::ROTATE_ROW ? 2 * (u64)c.n - 1
                                                                  : (kd->fhe_prop->p ? kd->fhe_prop->p->galois_element : 0);
            LSA_REQUIRE(gel != 0, "Galois element missing on the key datum");
            els.push_back(gel);
            keys.push_back(&std::any_cast<KeyP>(avail.at(kd->index))->key);
            slabs.push_back(ln.dslab(w * m));
            outs.push_back(slabs.back()->ptr);
        }
        if (g.algo == ALGO_BFV)
            bfv_rotate_many(c, lvl, a.ptr, (int)els.size(), els.data(), keys.data(), outs.data(), m, a.stride, (long long)w, s);
        else
            ckks_rotate_many(c, lvl, a.ptr, (int)els.size(), els.data(), keys.data(), outs.data(), m, a.stride, (long long)w, s);
        for (size_t gi = 0; gi < group->size(); gi++) {
            auto& mn = buckets[*(*group)[gi]];
            publish(avail, slabs[gi], (size_t)m, DevDatum{nullptr, nullptr, 2, lvl, false}, N, [&](size_t i) { return mn[i]; });
            ln.defer(slabs[gi]);
            gpu_nodes += m;
            done.insert((*group)[gi]);
        }
        gpu_batches++;
    }
}

Split Dispatcher::split(const std::vector<ComputeNode*>& level) const {
    Split sp;
    for (ComputeNode* n : level) {
        if (n->on_cpu) sp.cpu.push_back(n);
        else if (n->op() == OperationType::LOAD_TO_BACKEND) sp.loads.push_back(n);
        else if (n->op() == OperationType::STORE_FROM_BACKEND) sp.stores.push_back(n);
        else {
            const std::string sg = signature(n);
            if (!sp.buckets.count(sg)) sp.bucket_order.push_back(sg);
            sp.buckets[sg].push_back(n);
        }
    }
    return sp;
}

}  // namespace task
}  // namespace lsa
