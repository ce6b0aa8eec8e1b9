"""The host-side steps every pass over a finished map takes, owned once: ``fit_lists`` renders until a camera's per-tile lists fit,
``run_pass`` enqueues one render per item with no host read in between, reads once and repeats the items that were flagged.  Plain
Python: the callers (``FusedEngine.relearn_lists`` / ``add_new_gaussians``, ``evaluation``, ``mesh``, ``view.render_trajectory``) bring
the renders, the tables and the reads."""
from __future__ import annotations


def fit_lists(render, digest, what, tries=3):
    """``render()`` until its lists fitted -- ``digest()``, which re-sizes them, says whether they overflowed -- ``tries`` times at
    most; then RuntimeError(``what``)."""
    for _ in range(tries):
        render()
        if not digest():
            return
    raise RuntimeError(what)


def run_pass(items, enqueue, read, redo):
    """``enqueue(n, item)`` for every item in order (nothing may read the device there), then ``read()`` ONCE: the host read of the
    pass, which returns the indices n of the items whose lists did not fit; those get ``redo(n, item)`` in item order.  Returns the
    items that were repeated."""
    items = list(items)
    for n, item in enumerate(items):
        enqueue(n, item)
    flagged = sorted(read())
    for n in flagged:
        redo(n, items[n])
    return [items[n] for n in flagged]
