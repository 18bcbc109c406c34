"""Launch arithmetic of the key-switch family that depends on the batch alone, restated in plain Python, and the batch builder of
tests/test_gpu_batch_regimes.py.

  ks_mac_groups / mac_gx   lattisense_amd/csrc/ks_mac_groups.h (tests/test_ks_mac_groups_host.py holds the two together)
  tile_cap / auto_tile     pick_tile of lattisense_amd/csrc/key_switch.hip with lsa_set_tile_batch(0)
  spread                   a batch drawn from a few distinct ciphertexts, so that a large batch costs few oracle runs and
                           every position is still compared with the oracle"""
import numpy as np

FILL_WORKGROUPS = 2048          # KS_MAC_FILL_WORKGROUPS
TPB = 256                       # threads per workgroup of the element-wise kernels, two points per thread
WORKSPACE_CAP = 8 << 30         # bytes of operator workspace an automatic tile may take
MIN_SPREAD = 30                 # fewest batch positions a spread batch may have (below)


def mac_gx(n, targets):
    """grid.x of the stand-alone key MAC: one workgroup per 512 points of every target limb"""
    return targets * (n // (2 * TPB))


def ks_mac_groups(gx, batch):
    """(groups, bpt, gy): group y walks the items [y * bpt, min(batch, (y + 1) * bpt))"""
    groups = max(1, min(batch, -(-FILL_WORKGROUPS // gx)))
    bpt = -(-batch // groups)
    return groups, bpt, -(-batch // bpt)


def short_last_group(gx, batch):
    """several items per group, several groups, and a last group that is shorter than the others"""
    _, bpt, gy = ks_mac_groups(gx, batch)
    return 2 <= bpt < batch and batch % bpt != 0 and gy >= 2


def tile_cap(n):
    return min(512, max(64, (64 << 16) // n))


def auto_tile(n, rows_per_ct, batch):
    tb = max(1, WORKSPACE_CAP // max(rows_per_ct * n * 8, 1))
    return min(tb, tile_cap(n), batch)


def ks_tile_rows(level, n_special):
    """KsTile::rows for an NTT-domain source: workspace rows of N words per batch item of one key switch (cx, the extended
    digits, the extended accumulator, ModDown's conversions)"""
    L = level + 1
    T = L + n_special
    return L + -(-L // n_special) * T + 2 * T + 2 * L


def hmult_rows(level, n_special, fold):
    """workspace rows per batch item of lsa_ckks_mult_relin_rescale (ops.hip): d3 unless the tensor product is folded into the key
    switch, the relinearised pair, and the key switch's rows shared with the rescale's"""
    L = level + 1
    return (0 if fold else 3 * L) + 2 * L + max(ks_tile_rows(level, n_special), 2 * (1 + level))


# (gx, batch) of every stand-alone key MAC that tests/test_gpu_batch_regimes.py launches on purpose: the host test prints the
# header's triples for these and compares them with ks_mac_groups above
SHAPES = (
    (mac_gx(1 << 12, 7), 39), (mac_gx(1 << 12, 7), 76),      # a, e, f: N = 2^12, 5 Q + 2 P
    (mac_gx(1 << 16, 8), 5),                                 # b: N = 2^16, 6 Q + 2 P
    (mac_gx(1 << 12, 5), 512), (mac_gx(1 << 12, 5), 1),      # d: N = 2^12, 3 Q + 2 P, batch 513 in tiles of 512 and 1
    (mac_gx(1 << 14, 5), 256), (mac_gx(1 << 14, 5), 1),      # d: N = 2^14
    (mac_gx(1 << 12, 3), 39),                                # f: BFV, 2 Q + 1 P
    (mac_gx(1 << 12, 4), 2),                                 # g: 3 Q + 1 P
    (mac_gx(1 << 16, 17), 48),                               # h: the headline shape (limbs the fused kernel leaves)
)


def spread(rng, distinct, batch):
    """(items [batch, ...], pick [batch]): item b is distinct[pick[b]], pick uniform over the K = len(distinct) sources with
    every source used and positions 0 and batch - 1 holding different ones.  An item that took a neighbour's data goes unseen
    with probability 1/K per item; at least MIN_SPREAD positions are compared, so a systematic mix-up cannot pass."""
    distinct = np.asarray(distinct)
    k = len(distinct)
    assert k >= 2 and batch >= MIN_SPREAD and batch >= k
    while True:
        pick = rng.integers(0, k, size=batch)
        if pick[0] != pick[-1] and len(set(pick.tolist())) == k:
            break
    return np.ascontiguousarray(distinct[pick]), pick
