"""numpy reference of rsk_deliver_batch / rsk_deliver_host (include/rsk_codec.h) and the random cases
the host and GPU delivery tests share: the expected arena is the payload slices concatenated in
delivery order (each followed by zeros up to its rounded length), the expected offsets np.cumsum of
the rounded lengths as uint64."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LENS = np.array([0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 1400, 1469], np.uint16)
ARENA = 1 << 18  # bytes of the random source arena; payloads may overlap in it
STRAY = 0xFFFFFFFF


@dataclass
class Case:
    arena: np.ndarray      # uint8
    base_off: np.ndarray   # uint64 [n]
    inner_off: np.ndarray | None  # uint16 [n]
    pay_off: np.ndarray    # uint16 [n]
    pay_len: np.ndarray    # uint16 [n]
    status: np.ndarray     # int8 [n]
    order: np.ndarray | None  # uint32 [n] (entries past n_order are stray)
    n_order: int | None

    @property
    def n(self) -> int:
        return len(self.status)


def make_case(n: int, seed: int, valid: float = 0.5, order: str = "none", inner: bool = True,
              lens: np.ndarray = LENS) -> Case:
    """n packets at random byte offsets of a random arena, lengths drawn from `lens`, a `valid` share
    of them VALID (the others DROP or CLOSE, with lengths that must be ignored).  order: "none",
    "valid_idx" (the VALID indices, increasing) or "subset" (a random duplicate-free subset of all
    indices, VALID or not, in random order)."""
    rng = np.random.default_rng(seed)
    arena = rng.integers(0, 256, ARENA, dtype=np.uint8)
    pay_len = rng.choice(lens, n).astype(np.uint16)
    pay_off = rng.integers(8, 64, n).astype(np.uint16)  # 8 + hlen, any alignment
    inner_off = rng.integers(0, 96, n).astype(np.uint16) if inner else None
    base_off = rng.integers(0, ARENA - 1469 - 64 - 96, n).astype(np.uint64)
    status = np.where(rng.random(n) < valid, 1, rng.choice(np.array([0, -1], np.int8), n)).astype(np.int8)
    if order == "none":
        return Case(arena, base_off, inner_off, pay_off, pay_len, status, None, None)
    if order == "valid_idx":
        idx = np.nonzero(status == 1)[0].astype(np.uint32)
    else:
        idx = rng.permutation(n)[: rng.integers(0, n + 1)].astype(np.uint32)
    full = np.full(n, STRAY, np.uint32)
    full[: len(idx)] = idx
    return Case(arena, base_off, inner_off, pay_off, pay_len, status, full, len(idx))


def lengths(c: Case) -> tuple[np.ndarray, np.ndarray]:
    """(L_k, source offset of payload k) for the n positions."""
    n = c.n
    m = n if c.order is None else min(int(c.n_order), n)
    idx = np.arange(n, dtype=np.int64) if c.order is None else c.order[:m].astype(np.int64)
    idx = idx[:m]
    ok = idx < n
    safe = np.where(ok, idx, 0)
    ok &= c.status[safe] == 1
    L = np.zeros(n, np.int64)
    L[:m] = np.where(ok, c.pay_len[safe].astype(np.int64), 0)
    src = np.zeros(n, np.int64)
    s = c.base_off[safe].astype(np.int64) + c.pay_off[safe].astype(np.int64)
    if c.inner_off is not None:
        s = s + c.inner_off[safe].astype(np.int64)
    src[:m] = np.where(ok, s, 0)
    return L, src


def expected(c: Case, align: int) -> tuple[np.ndarray, np.ndarray, int]:
    """(arena, out_off uint64 [n + 1], total) of a delivery of c with `align`."""
    L, src = lengths(c)
    R = (L + align - 1) // align * align
    off = np.concatenate([[0], np.cumsum(R.astype(np.uint64), dtype=np.uint64)]).astype(np.uint64)
    total = int(off[-1])
    out = np.zeros(total, np.uint8)
    sel = L > 0
    Ls = L[sel]
    if Ls.size:
        within = np.arange(int(Ls.sum()), dtype=np.int64) - np.repeat(np.cumsum(Ls) - Ls, Ls)
        out[np.repeat(off[:-1][sel].astype(np.int64), Ls) + within] = c.arena[np.repeat(src[sel], Ls) + within]
    return out, off, total
