"""An own-words model of process_registry_updates and process_slashings as the engine runs them over its resident arrays
(pe_registry_updates, pe_process_slashings).  The reference holds the fields (pe:36-45, `slashings` pe:359/397) and names
get_validator_churn_limit (pe:1261, 1270) without giving the two functions' text: the rules below are restated from the
consensus specification [UPSTREAM-MEMORY], as DESIGN.md section 6 tags the rewards and SSZ.

Two forms of each:
  *_sequential   the specification's loop, one validator after the other, Python integers
  *_numpy        what the kernels compute: predicates over whole arrays, the exit queue's closed form, the queue's head by
                 a stable sort
tests/test_registry_updates_model.py holds one to the other; the GPU tests compare the engine with the numpy form.

A registry is a dict of arrays, one entry per validator: elig, act, ext, wdr (the four epochs), eff (effective balance),
slashed (0/1), bal (balance).  ValueError = the call the engine refuses with PE_ERR_INVALID_ARG."""
import os
from dataclasses import asdict, dataclass

import numpy as np

FAR = 2**64 - 1
U64 = 2**64
ETH = 10**9
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "registry_updates_vectors.json")
FIELDS = ("elig", "act", "ext", "wdr", "eff", "slashed", "bal")
REGISTRY_STATS = ("n_active", "churn_limit", "activation_churn_limit", "n_marked_eligible", "n_ejected", "first_exit_epoch",
                  "last_exit_epoch", "queue_len", "n_activated", "activation_epoch")
SLASHINGS_STATS = ("total_active_balance", "adjusted_total_slashing_balance", "n_penalised", "penalties", "n_saturated")


@dataclass
class Params:
    """pe_registry_params, mainnet values; the activation cap 0 = none (before Deneb), Deneb: 8."""
    max_effective_balance: int = 32 * ETH
    ejection_balance: int = 16 * ETH
    max_seed_lookahead: int = 4
    min_validator_withdrawability_delay: int = 256
    min_per_epoch_churn_limit: int = 4
    churn_limit_quotient: int = 65536
    max_per_epoch_activation_churn_limit: int = 0

    def abi(self) -> dict:
        return asdict(self)


def copy_registry(a: dict) -> dict:
    return {k: np.array(a[k], dtype=np.uint8 if k == "slashed" else np.uint64) for k in FIELDS}


def churn_limits(n_active: int, p: Params):
    if p.churn_limit_quotient == 0:
        raise ValueError("churn_limit_quotient is 0")
    limit = max(p.min_per_epoch_churn_limit, n_active // p.churn_limit_quotient)
    if limit == 0:
        raise ValueError("the churn limit is 0")
    cap = p.max_per_epoch_activation_churn_limit
    return limit, (min(cap, limit) if cap else limit)


def activation_exit_epoch(cur: int, p: Params) -> int:
    e = cur + 1 + p.max_seed_lookahead
    if e >= FAR:
        raise ValueError("current_epoch + 1 + max_seed_lookahead reaches FAR_FUTURE_EPOCH")
    return e


# ------------------------------------------------------------------ process_registry_updates, the specification's loop
def registry_updates_sequential(a: dict, cur: int, fin: int, p: Params = Params()):
    """-> (the registry after the call, stats by the names of pe_registry_stats).  `a` is not written."""
    elig, act, ext, wdr, eff = ([int(x) for x in a[k]] for k in ("elig", "act", "ext", "wdr", "eff"))
    n = len(eff)
    n_active = sum(1 for v in range(n) if act[v] <= cur < ext[v])
    limit, activation_limit = churn_limits(n_active, p)
    target = activation_exit_epoch(cur, p)
    st = dict.fromkeys(REGISTRY_STATS, 0)
    st.update(n_active=n_active, churn_limit=limit, activation_churn_limit=activation_limit, activation_epoch=target)
    for v in range(n):
        if elig[v] == FAR and eff[v] == p.max_effective_balance:
            elig[v] = cur + 1
            st["n_marked_eligible"] += 1
        if act[v] <= cur < ext[v] and eff[v] <= p.ejection_balance:
            if ext[v] != FAR:            # initiate_validator_exit: an exit already under way
                continue
            q = max([e for e in ext if e != FAR] + [target])
            if sum(1 for e in ext if e == q) >= limit:
                q += 1
            if q + p.min_validator_withdrawability_delay >= FAR:
                raise ValueError("exit epoch + min_validator_withdrawability_delay reaches FAR_FUTURE_EPOCH")
            ext[v] = q
            wdr[v] = q + p.min_validator_withdrawability_delay
            if st["n_ejected"] == 0:
                st["first_exit_epoch"] = q
            st["last_exit_epoch"] = q
            st["n_ejected"] += 1
    queue = sorted((v for v in range(n) if elig[v] <= fin and act[v] == FAR), key=lambda v: (elig[v], v))
    st["queue_len"] = len(queue)
    for v in queue[:activation_limit]:
        act[v] = target
        st["n_activated"] += 1
    out = copy_registry(a)
    for k, x in (("elig", elig), ("act", act), ("ext", ext), ("wdr", wdr)):
        out[k] = np.array(x, dtype=np.uint64)
    return out, st


# ------------------------------------------------------------------ ... and what the kernels compute
def exit_queue_start(ext: np.ndarray, target: int, limit: int):
    """(base, fill): the epoch the next exit goes to and how many already leave then."""
    set_ = ext[ext != np.uint64(FAR)]
    e0, c0 = target, 0
    if set_.size and int(set_.max()) >= target:
        e0 = int(set_.max())
        c0 = int((set_ == np.uint64(e0)).sum())
    return (e0 + 1, 0) if c0 >= limit else (e0, c0)


def registry_updates_numpy(a: dict, cur: int, fin: int, p: Params = Params()):
    out = copy_registry(a)
    elig, act, ext, eff = out["elig"].copy(), out["act"].copy(), out["ext"].copy(), out["eff"]
    c, f, far = np.uint64(cur), np.uint64(fin), np.uint64(FAR)
    active = (act <= c) & (c < ext)
    n_active = int(active.sum())
    limit, activation_limit = churn_limits(n_active, p)
    target = activation_exit_epoch(cur, p)
    marked = (elig == far) & (eff == np.uint64(p.max_effective_balance))
    fresh = active & (eff <= np.uint64(p.ejection_balance)) & (ext == far)
    queued = (elig <= f) & (act == far)          # as read before the marks: a mark gives cur + 1 > fin
    st = dict.fromkeys(REGISTRY_STATS, 0)
    st.update(n_active=n_active, churn_limit=limit, activation_churn_limit=activation_limit, activation_epoch=target,
              n_marked_eligible=int(marked.sum()), n_ejected=int(fresh.sum()), queue_len=int(queued.sum()))
    base, fill = exit_queue_start(ext, target, limit)
    k = np.arange(st["n_ejected"], dtype=np.uint64)
    if k.size:
        last = base + (fill + int(k[-1])) // limit
        if last + p.min_validator_withdrawability_delay >= FAR:
            raise ValueError("exit epoch + min_validator_withdrawability_delay reaches FAR_FUTURE_EPOCH")
        q = np.uint64(base) + (np.uint64(fill) + k) // np.uint64(limit)
        out["ext"][fresh] = q
        out["wdr"][fresh] = q + np.uint64(p.min_validator_withdrawability_delay)
        st["first_exit_epoch"], st["last_exit_epoch"] = int(q[0]), int(q[-1])
    out["elig"][marked] = np.uint64(cur + 1)
    idx = np.flatnonzero(queued)
    head = idx[np.argsort(elig[idx], kind="stable")][:activation_limit]     # (eligibility epoch, index)
    out["act"][head] = np.uint64(target)
    st["n_activated"] = int(head.size)
    return out, st


# ------------------------------------------------------------------ process_slashings
def view_flags(a: dict, cur: int) -> np.ndarray:
    """The working-state view's flag byte: PE_VAL_ACTIVE (1), PE_VAL_SLASHED (2), PE_VAL_ACTIVE_PREV (8)."""
    prev = np.uint64(max(cur, 1) - 1)
    c = np.uint64(cur)
    return (((a["act"] <= c) & (c < a["ext"])).astype(np.uint8) | (a["slashed"].astype(np.uint8) << 1)
            | (((a["act"] <= prev) & (prev < a["ext"])).astype(np.uint8) << 3)).astype(np.uint8)


def slashings_scalars(total_active: int, cur: int, sum_slashings: int, multiplier: int, vector: int):
    scaled = sum_slashings * multiplier
    if scaled >= U64:
        raise ValueError("sum_slashings * multiplier exceeds 64 bits")
    if cur + vector // 2 >= U64:
        raise ValueError("current_epoch + vector / 2 exceeds 64 bits")
    return min(scaled, total_active), cur + vector // 2


def slashings_sequential(a: dict, flags, cur: int, sum_slashings: int, multiplier: int = 3, vector: int = 8192,
                         increment: int = ETH):
    """-> (balances after the call, stats by the names of pe_slashings_stats).  flags: the view's bytes (view_flags)."""
    eff, wdr, bal = ([int(x) for x in a[k]] for k in ("eff", "wdr", "bal"))
    total = max(increment, sum(eff[v] for v in range(len(eff)) if flags[v] & 1))
    adj, target = slashings_scalars(total, cur, sum_slashings, multiplier, vector)
    st = dict(total_active_balance=total, adjusted_total_slashing_balance=adj, n_penalised=0, penalties=0, n_saturated=0)
    for v in range(len(eff)):
        if (flags[v] & 2) and target == wdr[v]:
            numerator = eff[v] // increment * adj
            if numerator >= U64:
                raise ValueError("effective_balance / increment * adjusted exceeds 64 bits")
            penalty = numerator // total * increment
            if penalty > bal[v]:
                st["n_saturated"] += 1
                penalty = bal[v]
            bal[v] -= penalty
            st["n_penalised"] += 1
            st["penalties"] += penalty
    return np.array(bal, dtype=np.uint64), st


def slashings_numpy(a: dict, flags, cur: int, sum_slashings: int, multiplier: int = 3, vector: int = 8192,
                    increment: int = ETH):
    flags = np.asarray(flags, dtype=np.uint8)
    eff, bal = a["eff"], a["bal"].copy()
    total = max(increment, int(eff[(flags & 1) != 0].astype(object).sum()) if eff.size else 0)
    adj, target = slashings_scalars(total, cur, sum_slashings, multiplier, vector)
    hit = ((flags & 2) != 0) & (a["wdr"] == np.uint64(target))
    st = dict(total_active_balance=total, adjusted_total_slashing_balance=adj, n_penalised=int(hit.sum()), penalties=0,
              n_saturated=0)
    if hit.any():
        if int(eff[hit].max()) // increment * adj >= U64:
            raise ValueError("effective_balance / increment * adjusted exceeds 64 bits")
        penalty = eff[hit] // np.uint64(increment) * np.uint64(adj) // np.uint64(total) * np.uint64(increment)
        cut = np.minimum(penalty, bal[hit])
        st["n_saturated"] = int((penalty > bal[hit]).sum())
        st["penalties"] = int(cut.astype(object).sum())
        bal[hit] -= cut
    return bal, st


# ------------------------------------------------------------------ registries
def blank_registry(n: int, p: Params = Params()) -> dict:
    """n validators to which neither function does anything: active since epoch 0, full balances, nobody leaving, queued,
    waiting for a mark or slashed."""
    u = lambda x: np.full(n, x, dtype=np.uint64)  # noqa: E731
    return dict(elig=u(0), act=u(0), ext=u(FAR), wdr=u(FAR), eff=u(p.max_effective_balance), slashed=np.zeros(n, dtype=np.uint8),
                bal=u(p.max_effective_balance))


def exit_queue_case(n, cur, L, c0, e0_beyond, n_eject, interleave):
    """n validators, churn limit L, c0 validators already leaving at E0 (the look-ahead epoch, or one beyond it), n_eject
    fresh ejections spread over the registry, and between them ejection candidates whose exit is set."""
    p = Params(min_per_epoch_churn_limit=L)
    a = blank_registry(n, p)
    e0 = cur + 1 + p.max_seed_lookahead + (3 if e0_beyond else 0)
    a["ext"][n - c0:] = e0
    a["wdr"][n - c0:] = e0 + 256
    if e0_beyond:
        a["ext"][0] = e0 - 1                      # an earlier exit that must not count
    step = max(1, (n - c0 - 2) // max(1, n_eject))
    fresh = (1 + step * np.arange(n_eject))
    assert fresh.size == 0 or fresh[-1] < n - c0
    a["eff"][fresh] = p.ejection_balance
    if interleave:
        mid = fresh[:-1] + 1 if step > 1 else np.zeros(0, dtype=int)
        a["eff"][mid] = p.ejection_balance - 1
        a["ext"][mid] = cur + 2                   # still active at cur, exit already set: no-ops that must not advance k
    return a, p


def random_registry(n: int, seed: int, cur: int, fin: int, p: Params = Params(), vector: int = 8192):
    """-> (registry, counters).  Every class and every edge value, in any registry of at least 256 validators: the first 256
    walk the products of the edge lists, the rest draw from them.  cur >= 2, 1 <= fin <= cur."""
    assert cur >= 2 and 1 <= fin <= cur
    rng = np.random.default_rng(seed)
    half = cur + vector // 2
    effs = [p.ejection_balance - 1, p.ejection_balance, p.ejection_balance + 1, p.max_effective_balance - 1,
            p.max_effective_balance]
    acts = [cur - 1, cur, cur + 1, 0, FAR]
    exts = [cur - 1, cur, cur + 1, FAR, cur + 9]
    eligs = [fin - 1, fin, fin + 1, FAR]
    wdrs = [half - 1, half, half + 1]
    v = np.arange(n)
    walk = v < 256
    draw = lambda m: rng.integers(0, m, size=n)  # noqa: E731
    i_eff = np.where(walk, v % 5, draw(5))
    i_act = np.where(walk, (v // 5) % 5, draw(5))
    i_ext = np.where(walk, (v // 25) % 5, np.where(draw(4) == 0, draw(5), 3))  # beyond the walk three exits in four are open
    i_elig = np.where(walk, v % 4, draw(4))
    slashed = np.where(walk, (v % 7 < 3), draw(8) == 0).astype(np.uint8)
    i_wdr = np.where(walk, (v // 7) % 3, draw(3))
    take = lambda vals, i: np.array(vals, dtype=np.uint64)[i]  # noqa: E731
    a = dict(elig=take(eligs, i_elig), act=take(acts, i_act), ext=take(exts, i_ext), eff=take(effs, i_eff), slashed=slashed)
    # withdrawable: the three neighbours of the target for every other validator, slashed or not; else what an exit implies
    at_target = (v % 2 == 0)
    implied = np.where(a["ext"] == np.uint64(FAR), np.uint64(FAR), a["ext"] + np.uint64(p.min_validator_withdrawability_delay))
    a["wdr"] = np.where(at_target, take(wdrs, i_wdr), implied).astype(np.uint64)
    # balances around the effective balance, and a few too small for any penalty
    a["bal"] = (a["eff"] + rng.integers(0, ETH, size=n, dtype=np.uint64)).astype(np.uint64)
    a["bal"][v % 11 == 0] = rng.integers(0, 1000, size=int((v % 11 == 0).sum()), dtype=np.uint64)
    a = copy_registry(a)
    c, f, far = np.uint64(cur), np.uint64(fin), np.uint64(FAR)
    active = (a["act"] <= c) & (c < a["ext"])
    low = a["eff"] <= np.uint64(p.ejection_balance)
    hit = (a["slashed"] != 0)
    counters = dict(
        marked=int(((a["elig"] == far) & (a["eff"] == np.uint64(p.max_effective_balance))).sum()),
        unmarked_short=int(((a["elig"] == far) & (a["eff"] == np.uint64(p.max_effective_balance - 1))).sum()),
        ejected=int((active & low & (a["ext"] == far)).sum()),
        eject_exit_set=int((active & low & (a["ext"] != far)).sum()),
        not_ejected_above=int((active & (a["eff"] == np.uint64(p.ejection_balance + 1))).sum()),
        low_not_active=int((~active & low).sum()),
        exits_set=int((a["ext"] != far).sum()),
        queued=int(((a["elig"] <= f) & (a["act"] == far)).sum()),
        queued_at_fin=int(((a["elig"] == f) & (a["act"] == far)).sum()),
        not_queued_after_fin=int(((a["elig"] == np.uint64(fin + 1)) & (a["act"] == far)).sum()),
        not_queued_activated=int(((a["elig"] <= f) & (a["act"] != far)).sum()),
        slashed_before=int((hit & (a["wdr"] == np.uint64(half - 1))).sum()),
        slashed_at=int((hit & (a["wdr"] == np.uint64(half))).sum()),
        slashed_after=int((hit & (a["wdr"] == np.uint64(half + 1))).sum()),
        unslashed_at=int((~hit & (a["wdr"] == np.uint64(half))).sum()),
    )
    for edge in (cur - 1, cur, cur + 1):
        counters[f"act_{edge - cur:+d}"] = int((a["act"] == np.uint64(edge)).sum())
        counters[f"ext_{edge - cur:+d}"] = int((a["ext"] == np.uint64(edge)).sum())
    return a, counters


def every_class_occurred(counters: dict) -> bool:
    return all(x > 0 for x in counters.values())
