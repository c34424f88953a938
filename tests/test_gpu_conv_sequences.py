"""GPU: rsk_control_batch and rsk_conv_resolve_batch alternating on one stream, batch sizes up and down
(120,000 / 2,049 / 70,000 / 1): both keep their tile counts in the same per-stream scratch (WS_CONTROL),
which grows at the first call and is reused, smaller, by the later ones.  Every call's lists equal the
restatements (tests/control_ref, tests/conv_ref).  Then the same on two streams at once, one host thread
each: calls on different streams never share scratch."""
from __future__ import annotations

import threading

import numpy as np
import pytest

from rsock_amd import codec as rc
from tests import control_ref as C
from tests import conv_ref as R

pytestmark = pytest.mark.gpu

SIZES = (120000, 2049, 70000, 1)


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(b"hello135", 0)
    yield c
    c.close()


def cases(seed):
    """Per size: a control case and a conv case, with their tables' columns."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        c, cols, cap = C.random_batch(rng, n, ctrl=0.3, capacity=257)
        vcols, vc = R.random_case(rng, n, 257, True, True, known=0.7, pool=100)
        out.append(((c, cols, cap), (vcols, vc)))
    return out


def alternate(cx, gpu, prepared, stream):
    import torch

    with torch.cuda.stream(stream):
        for (c, cols, cap), (vcols, vc) in prepared:
            got, want, _tab, _tmap = C.check_case(rc, c, cols, cap, False, gpu, cx)
            assert got["n_msg"] == want["n_msg"] and (got["n_msg"] > 0 or len(c["status"]) == 1)
            got, want, _tab = R.check_case(rc, vcols, vc, True, True, gpu, cx)
            assert got["n_msg"] == want["n_unknown"] and (got["n_msg"] > 0 or len(vc["status"]) == 1)


def test_control_and_conv_alternate_on_one_stream(cx, gpu):
    import torch

    alternate(cx, gpu, cases(1), torch.cuda.Stream(gpu))


def test_control_and_conv_on_two_streams_at_once(cx, gpu):
    import torch

    prepared = [cases(2), cases(3)[::-1]]  # the second stream walks the sizes the other way round
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(gpu)
            alternate(cx, gpu, prepared[k], streams[k])
        except BaseException as e:  # noqa: BLE001 - reported on the test's thread below
            errors.append((k, e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0][1]
