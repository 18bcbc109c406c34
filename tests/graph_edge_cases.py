"""The case table of tests/test_graph_synth_host.py and tests/test_gpu_graph_edges.py: hand-built task graphs
(tests/graph_synth.py) at the edge of every load-time rewrite and of the dispatcher's bucket, gather, hoisting and lifetime
logic.  N = 4096, levels <= 4, at most 33 terms.

Per case, written down by hand from the rules and not from a run:

  delta   (data, compute): counts() with the rewrites on minus counts() under LSA_NO_GRAPH_FUSION=1.  The ABI bridge nodes
          are the same in both modes (no rewrite adds or removes a task input or output), so this is the rewrites' own effect:
            mult -> relin -> rescale fused:      3 nodes -> 1, two intermediates gone                        (-2, -2)
            accumulation tree, P products, o (0 or 1) other operands, K = ceil(P / 16) chained MAC nodes:
                P products and P + o - 1 adds -> K nodes; P products and P + o - 2 inner sums -> K - 1 clones
                                                                                     (-2P - o + 1 + K) for both
            rotate-and-MAC, R private rotations (+1 if a product is absorbed): MAC + R (+1) nodes -> 1        (-R, -R)
  fused   (gpu_nodes, gpu_batches) of a run with the rewrites on
  plain   (gpu_nodes, gpu_batches) of a run under LSA_NO_GRAPH_FUSION=1
          gpu_nodes: the backend nodes (everything but the bridges).  gpu_batches: one per (level, signature) bucket, a
          hoisted rotation group counting once.  Task inputs are on the device after level 1 (export, load), so a node's
          level is 2 + its depth in the graph as written.
  components  independent subgraphs (>= 2: the case also runs under LSA_PIPELINE_MIN_MIB=0; the plan pipelines from 4 on)
"""
import collections

from tests.graph_synth import Graph

Case = collections.namedtuple("Case", "name build delta fused plain components")
CASES = []


def case(name, delta, fused, plain, components=1):
    def reg(fn):
        CASES.append(Case(name, fn, (delta, delta) if isinstance(delta, int) else delta, fused, plain, components))
        return fn
    return reg


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---------------------------------------------------------------------------------------------------- A: mult -> relin -> rescale
def _chain(g, x, y, k):
    m = g.mult(x, y)
    r = g.relin(m, k)
    return m, r, g.rescale(r)


@case("A1_product_is_output", 0, (3, 3), (3, 3))
def a1():
    g = Graph("CKKS")
    m, _, z = _chain(g, g.ct(2), g.ct(2), g.rlk(2))
    g.output(m)
    g.output(z)
    return g


@case("A2_relin_second_reader", 0, (4, 4), (4, 4))   # rescale and add share a level: two buckets
def a2():
    g = Graph("CKKS")
    x, y, c, k = g.ct(2), g.ct(2), g.ct(2), g.rlk(2)
    _, r, z = _chain(g, x, y, k)
    g.output(g.add(r, c))
    g.output(z)
    return g


@case("A3_relin_is_output", 0, (3, 3), (3, 3))
def a3():
    g = Graph("CKKS")
    _, r, z = _chain(g, g.ct(2), g.ct(2), g.rlk(2))
    g.output(r)
    g.output(z)
    return g


# squares written mult [x] (twice) and mult [x, x] (twice): four components.  Fused: the two forms have different signatures
# (2 and 3 inputs), two buckets of two.  Plain: mult in two buckets, relin and rescale in one each.
@case("A4_squares", -8, (4, 2), (12, 4), components=4)
def a4():
    g = Graph("CKKS")
    xs = [g.ct(2) for _ in range(4)]
    k = g.rlk(2)
    for i, x in enumerate(xs):
        g.output(_chain(g, x, x if i & 1 else None, k)[2])
    return g


@case("A5_level1", -2, (1, 1), (3, 3))
def a5():
    g = Graph("CKKS")
    z = _chain(g, g.ct(1), g.ct(1), g.rlk(1))[2]
    assert g.level(z) == 0
    g.output(z)
    return g


@case("A6_shared_operands", -4, (2, 1), (6, 3))
def a6():
    g = Graph("CKKS")
    x, y, k = g.ct(2), g.ct(2), g.rlk(2)
    g.output(_chain(g, x, y, k)[2])
    g.output(_chain(g, x, y, k)[2])
    return g


@case("A7_key_two_levels_up", -2, (1, 1), (3, 3))
def a7():
    g = Graph("CKKS")
    g.output(_chain(g, g.ct(2), g.ct(2), g.rlk(4))[2])
    return g


# three chains in one level whose first operands are a task input, a device result, a task input (the other operand of the
# first and third is a device result, so that all three sit one level below the negations).  3 neg (one bucket) + 3 chains.
def _a8(reverse):
    g = Graph("CKKS")
    x = [g.ct(2) for _ in range(3)]
    y = [g.ct(2) for _ in range(3)]
    k = g.rlk(2)
    n0, n1, n2 = g.neg(y[0]), g.neg(x[1]), g.neg(y[2])
    for a, b in ((x[0], n0), (n1, y[1]), (x[2], n2)):
        g.output(_chain(g, a, b, k)[2])
    if reverse:
        g.reverse_compute_order()
    return g


case("A8_mixed_sources", -6, (6, 2), (12, 4), components=3)(lambda: _a8(False))
case("A8_mixed_sources_reversed", -6, (6, 2), (12, 4), components=3)(lambda: _a8(True))


# ---------------------------------------------------------------------------------------------------- B: accumulation trees
def _sum_chain(g, items):
    s = items[0]
    for it in items[1:]:
        s = g.add(s, it)
    return s


def _sum_tree(g, items):
    """pairwise, layer by layer; an odd one out is carried to the next layer as the last item, so every add of a layer has an
    operand from the layer below and all of them sit in one level"""
    items, layers = list(items), 0
    while len(items) > 1:
        nxt = [g.add(items[i], items[i + 1]) for i in range(0, len(items) - 1, 2)]
        if len(items) & 1:
            nxt.append(items[-1])
        items, layers = nxt, layers + 1
    return items[0], layers


def _products(g, n, level, plain):
    return [g.mult(g.ct(level), plain(i)) for i in range(n)]


def _b1(P, tree, other):
    def build():
        g = Graph("CKKS")
        items = _products(g, P, 2, lambda i: g.pt(2))
        if other:
            items = [g.ct(2)] + items if not tree else items + [g.ct(2)]
        g.output(_sum_tree(g, items)[0] if tree else _sum_chain(g, items))
        return g
    K = -(-P // 16)
    leaves = P + other
    # plain: the products are one bucket; a chain's adds sit in a level each, a tree's in ceil(log2(leaves)) layers
    add_batches = (leaves - 1).bit_length() if tree else leaves - 1
    case("B1_%s_%d%s" % ("tree" if tree else "chain", P, "_other" if other else ""),
         -2 * P - other + 1 + K, (K, K), (2 * P + other - 1, 1 + add_batches))(build)


for _P in (2, 16, 17, 33):
    for _tree in (False, True):
        for _other in (0, 1):
            _b1(_P, _tree, _other)


# four independent 2-product sums: one bucket of four MACs; plain: a bucket of 8 products, a bucket of 4 adds
@case("B1_four_components", -8, (4, 1), (12, 2), components=4)
def b1x4():
    g = Graph("CKKS")
    for _ in range(4):
        g.output(_sum_chain(g, _products(g, 2, 2, lambda i: g.pt(2))))
    return g


@case("B2_two_others", 0, (5, 4), (5, 4))
def b2():
    g = Graph("CKKS")
    p = _products(g, 2, 2, lambda i: g.pt(2))
    g.output(_sum_chain(g, p + [g.ct(2), g.ct(2)]))
    return g


# p0 is also negated: it stays and becomes the partial sum of a 2-term MAC.  Fused: mult | neg, MAC.  Plain: 3 mult | add, neg | add
@case("B3_one_shared_product", -3, (3, 3), (6, 4))
def b3a():
    g = Graph("CKKS")
    p = _products(g, 3, 2, lambda i: g.pt(2))
    g.output(_sum_chain(g, p))
    g.output(g.neg(p[0]))
    return g


@case("B3_two_shared_products", 0, (7, 4), (7, 4))   # 3 mult | add, 2 neg | add
def b3b():
    g = Graph("CKKS")
    p = _products(g, 3, 2, lambda i: g.pt(2))
    g.output(_sum_chain(g, p))
    g.output(g.neg(p[0]))
    g.output(g.neg(p[1]))
    return g


@case("B3_product_is_output", -3, (2, 2), (5, 3))
def b3c():
    g = Graph("CKKS")
    p = _products(g, 3, 2, lambda i: g.pt(2))
    g.output(p[0])
    g.output(_sum_chain(g, p))
    return g


# a level-3 product dropped to level 2 is not a product of the tree: it is the partial sum.
# Fused: mult@3 | drop | MAC.  Plain: mult@3, 2 mult@2 | drop, add | add
@case("B4_product_above_root", -3, (3, 3), (6, 5))
def b4():
    g = Graph("CKKS")
    hi = g.mult(g.ct(3), g.pt(3))
    p = _products(g, 2, 2, lambda i: g.pt(2))
    g.output(_sum_chain(g, p + [g.drop_level(hi, 2)]))
    return g


@case("B5_one_ciphertext", -4, (1, 1), (5, 3))
def b5a():
    g = Graph("CKKS")
    x = g.ct(2)
    g.output(_sum_chain(g, [g.mult(x, g.pt(2)) for _ in range(3)]))
    return g


@case("B5_one_plaintext", -4, (1, 1), (5, 3))
def b5b():
    g = Graph("CKKS")
    p = g.pt(2)
    g.output(_sum_chain(g, [g.mult(g.ct(2), p) for _ in range(3)]))
    return g


@case("B5_product_read_twice", 0, (4, 3), (4, 3))   # p0 + p0 + p1: p0 has two readers, both occurrences are "others"
def b5c():
    g = Graph("CKKS")
    p = _products(g, 2, 2, lambda i: g.pt(2))
    g.output(g.add(g.add(p[0], p[0]), p[1]))
    return g


# a1 = p0 + p1 is an output: a root of its own (2-term MAC) and the partial sum of the root above it (p2, p3)
@case("B6_inner_add_is_output", -5, (2, 2), (7, 4))
def b6a():
    g = Graph("CKKS")
    p = _products(g, 4, 2, lambda i: g.pt(2))
    a1 = g.output(g.add(p[0], p[1]))
    g.output(g.add(g.add(a1, p[2]), p[3]))
    return g


@case("B6_root_read_by_sub", -2, (2, 2), (4, 3))
def b6b():
    g = Graph("CKKS")
    p = _products(g, 2, 2, lambda i: g.pt(2))
    g.output(g.sub(g.add(p[0], p[1]), g.ct(2)))
    return g


def _flavours(algorithm, level, kinds):
    g = Graph(algorithm)
    mk = {"pt": lambda: g.pt(level), "ringt": g.pt_ringt, "mul": lambda: g.pt_mul(level)}
    g.output(_sum_chain(g, [g.mult(g.ct(level), mk[k]()) for k in kinds]))
    return g


# level 0 is where a ring-t plaintext's declared level equals the ciphertext's, so where its products first qualify.
# Plain: one product bucket per flavour, then the adds.
case("B7_ckks_pt_ringt_pt_l0", -4, (1, 1), (5, 4))(lambda: _flavours("CKKS", 0, ("pt", "ringt", "pt")))
case("B7_bfv_ringt_l0", -4, (1, 1), (5, 3))(lambda: _flavours("BFV", 0, ("ringt",) * 3))
case("B7_bfv_mul_l0", -4, (1, 1), (5, 3))(lambda: _flavours("BFV", 0, ("mul",) * 3))
# BFV runs a multiply-accumulate of pt_mul terms or of none: the two pt_mul products join, the ring-t product is the partial sum
case("B7_bfv_mul_ringt_mul_l0", -3, (2, 2), (5, 4))(lambda: _flavours("BFV", 0, ("mul", "ringt", "mul")))
case("B7_bfv_ringt_mul_l0", 0, (3, 3), (3, 3))(lambda: _flavours("BFV", 0, ("ringt", "mul")))
# three ring-t products join, the pt_mul product is the partial sum.  Plain: 2 product buckets + 3 adds
case("B7_bfv_ringt3_mul_l0", -5, (2, 2), (7, 5))(lambda: _flavours("BFV", 0, ("ringt", "ringt", "mul", "ringt")))
# two of each: neither flavour can take the other two as ONE partial sum, the tree stays
case("B7_bfv_two_of_each_l0", 0, (7, 5), (7, 5))(lambda: _flavours("BFV", 0, ("ringt", "mul", "mul", "ringt")))
# at level 2 a ring-t product never qualifies (declared level 0)
case("B7_bfv_mul_ringt_mul_l2", -3, (2, 2), (5, 4))(lambda: _flavours("BFV", 2, ("mul", "ringt", "mul")))
case("B7_bfv_ringt_mul_l2", 0, (3, 3), (3, 3))(lambda: _flavours("BFV", 2, ("ringt", "mul")))


# ---------------------------------------------------------------------------------------------------- C: BFV rotate-and-MAC
@case("C1_rotation_read_twice", 0, (2, 2), (2, 2))   # the rotation has two readers (both this MAC): not private, terms x and r differ
def c1():
    g = Graph("BFV")
    x = g.ct(2)
    r = g.rotate_col(x, g.glk(5, 2))
    g.output(g.cmp_sum([x, r, r], [g.pt_mul(2) for _ in range(3)]))
    return g


@case("C2_two_elements", -2, (1, 1), (3, 2))   # plain: both rotations of x hoist into one batch
def c2():
    g = Graph("BFV")
    x = g.ct(2)
    g.output(g.cmp_sum([g.rotate_col(x, g.glk(5, 2)), g.rotate_col(x, g.glk(25, 2))], [g.pt_mul(2), g.pt_mul(2)]))
    return g


# the partial sum is y * pt_mul, y another ciphertext: kept as the node's partial sum.  Fused: mult | rotate+MAC.  Plain: rot, mult | MAC
@case("C3_partial_of_other_ct", -1, (2, 2), (3, 3))
def c3():
    g = Graph("BFV")
    x, y = g.ct(2), g.ct(2)
    part = g.mult(y, g.pt_mul(2))
    g.output(g.cmpac_sum([g.rotate_col(x, g.glk(5, 2)), x], part, [g.pt_mul(2), g.pt_mul(2)]))
    return g


@case("C4_one_term", -1, (1, 1), (2, 2))
def c4():
    g = Graph("BFV")
    g.output(g.cmp_sum([g.rotate_col(g.ct(2), g.glk(5, 2))], [g.pt_mul(2)]))
    return g


# terms r1 = rot5(x) and rot25(r1): r1 has two readers and is the node's X, only the outer rotation is folded in
@case("C5_rotation_of_rotation", -1, (2, 2), (3, 3))
def c5():
    g = Graph("BFV")
    r1 = g.rotate_col(g.ct(2), g.glk(5, 2))
    g.output(g.cmp_sum([r1, g.rotate_col(r1, g.glk(25, 2))], [g.pt_mul(2), g.pt_mul(2)]))
    return g


# ---------------------------------------------------------------------------------------------------- D: buckets, hoisting, lifetimes
# elements 5 and 25 over [x0, x1] hoist together; element 125 over [x1, x0] (its x1 node has the lower compute index) is alone
@case("D1_hoist_by_input_order", 0, (6, 2), (6, 2), components=2)
def d1():
    g = Graph("CKKS")
    x0, x1 = g.ct(2), g.ct(2)
    k5, k25, k125 = g.glk(5, 2), g.glk(25, 2), g.glk(125, 2)
    for k in (k5, k25):
        g.output(g.rotate_col(x0, k))
        g.output(g.rotate_col(x1, k))
    g.output(g.rotate_col(x1, k125))
    g.output(g.rotate_col(x0, k125))
    return g


@case("D2_row_and_col_hoisted", 0, (2, 1), (2, 1))
def d2():
    g = Graph("BFV")
    x = g.ct(2)
    g.output(g.rotate_row(x, g.glk(2 * g.n - 1, 2)))
    g.output(g.rotate_col(x, g.glk(5, 2)))
    return g


@case("D3_rotation_chain", 0, (2, 2), (2, 2))
def d3():
    g = Graph("CKKS")
    r1 = g.output(g.rotate_col(g.ct(2), g.glk(5, 2)))
    g.output(g.rotate_col(r1, g.glk(25, 2)))
    return g


# a = -x is read one level later and again five levels after that; two degree-2 products come and go in between
@case("D4_long_lived_datum", 0, (7, 7), (7, 7))
def d4():
    g = Graph("CKKS")
    x, y, k = g.ct(2), g.ct(2), g.rlk(2)
    a = g.neg(x)
    b = g.add(a, y)
    r1 = g.relin(g.mult(b, y), k)
    r2 = g.relin(g.mult(r1, y), k)
    g.output(g.add(r2, a))
    return g


# a = -x is read twice by an add and twice by a mult in one level, and once more two levels later.  neg | add, mult | relin | add
@case("D5_read_twice_by_one_node", 0, (5, 5), (5, 5))
def d5():
    g = Graph("CKKS")
    a = g.neg(g.ct(2))
    g.output(g.add(a, a))
    r = g.relin(g.mult(a, a), g.rlk(2))
    g.output(g.add(r, a))
    return g


@case("D6_operand_shared_by_two_of_three", 0, (3, 1), (3, 1), components=2)
def d6():
    g = Graph("CKKS")
    x0, x1 = g.ct(2), g.ct(2)
    for x in (x0, x0, x1):
        g.output(g.add(x, g.ct(2)))
    return g
