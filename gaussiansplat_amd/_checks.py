"""Argument checks of the host mirror, each written once.  `who` / `what` is the caller's prefix: the messages are the callers' own."""
from __future__ import annotations

import math


def positive(what: str, v, allow_zero: bool = False) -> float:
    """v as a finite float > 0 (allow_zero: >= 0, which is a learning rate)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, got {v!r}") from None
    if not math.isfinite(f) or f < 0.0 or (f == 0.0 and not allow_zero):
        raise ValueError(f"{what} must be finite and {'>= 0' if allow_zero else '> 0'}, got {f}")
    return f


def probability(what: str, v) -> float:
    f = positive(what, v)
    if not f < 1.0:
        raise ValueError(f"{what} must lie in (0, 1), got {f}")
    return f


def logit(p: float) -> float:
    return math.log(p / (1.0 - p))


def integer(who: str, name: str, v, lo: int, strict: bool = False) -> int:
    """v as an integer >= lo, never a bool.  strict: an int itself (the schedules of the density controllers); else any number equal to one."""
    if isinstance(v, bool) or (not isinstance(v, int) if strict else int(v) != v) or v < lo:
        if strict:
            raise ValueError(f"{who}: {name} must be an integer >= {lo}, got {v!r}")
        raise ValueError(f"{who}: {name} must be {'a positive integer' if lo == 1 else f'an integer >= {lo}'}, not {v!r}")
    return int(v)


def betas_eps(who: str, betas, eps, got: bool = True) -> tuple:
    """Adam's ((beta1, beta2), eps) as floats: betas in [0, 1), eps finite and > 0.  got: the messages end with the offending value."""
    b1, b2 = (float(b) for b in betas)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"{who}: betas must lie in [0, 1)" + (f", got {tuple(betas)}" if got else ""))
    eps = float(eps)
    if not math.isfinite(eps) or eps <= 0.0:
        raise ValueError(f"{who}: eps must be finite and > 0" + (f", got {eps}" if got else ""))
    return (b1, b2), eps
