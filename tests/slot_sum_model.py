"""CPU restatement of the CKKS slot sum (lattisense_amd/csrc/slot_sum.h and slot_sum.hip slot_sum_run) over
oracle/ckks_bootstrap.py's Evaluator: the plan rule written out again, and its steps replayed with rotate_ext, add_ext, moddown and
add exactly as the operator states them.  The device gives these words."""


def steps_of(n_ring, step, count, radix=2):
    """[[(rotation mod N/2, "tail" | "next"), ...], ...]: one list per step (one decomposition), the TAIL key first"""
    h = n_ring // 2
    s, n, steps = step % h, count, []
    while n > 1:
        keys = []
        if n % 2:
            keys.append(((n - 1) * s % h, "tail"))
            n -= 1
        if radix == 4 and n % 4 == 0:
            keys += [(i * s % h, "next") for i in (1, 2, 3)]
            s, n = 4 * s % h, n // 4
        else:
            keys.append((s, "next"))
            s, n = 2 * s % h, n // 2
        assert all(r for r, _ in keys), "a planned rotation is a multiple of N/2"
        steps.append(keys)
    return steps


def rotations_of(n_ring, step, count, radix=2):
    return sorted({r for keys in steps_of(n_ring, step, count, radix) for r, _ in keys})


def slot_sum(ev, ct, step, count, radix=2):
    """ev: oracle.ckks_bootstrap.Evaluator, ct: its Ct.  x <- x + ModDown(sum of the step's NEXT extended rotations); the TAIL
    rotations gather over Q_level u P and are divided once at the end: out = x + ModDown(tail)."""
    x, tail = ct, None
    for keys in steps_of(ev.n, step, count, radix):
        nxt = None
        for r, dest in keys:
            e = ev.rotate_ext(x, r)
            if dest == "tail":
                tail = e if tail is None else ev.add_ext(tail, e)
            else:
                nxt = e if nxt is None else ev.add_ext(nxt, e)
        x = ev.add(x, ev.moddown(nxt))
    return x if tail is None else ev.add(x, ev.moddown(tail))
