"""Which refusal wins when a call of the group, NEES or sample families has two faults at once (include/fbus_ekf.h: the argument check
runs in a fixed order), and the two rules that are no refusal: group_mix runs with both outputs NULL, a host form inside a capture is
refused even when it asks for no output.  One table: (entry point, arguments with two faults, inside a capture or not) -> (return code,
what fbus_ekf_last_error must say, what it must not say).  Nothing is launched by a refused call: the records are compared after each.

The expectations are those of the library as it stood before these entry points shared one host wrapper."""
import ctypes as C

import numpy as np
import pytest
import torch

from support import make_filter, pose_setup

pytestmark = pytest.mark.gpu

B, N, G = 8, 18, 2
OVERLAP, CAPTURE = "overlaps the records", "not between graph_begin and graph_end"


class Env:
    """one fp32 handle with the likelihood sums off, and good arguments of every kind on the host and on the device"""

    def __init__(self, f):
        rng = np.random.default_rng(77)
        self.f = f
        self.recs = C.c_void_p(f.records()[0] + 64)                    # a device pointer inside the records
        self.truth, self.xi = rng.normal(size=(B, 19)), rng.normal(size=(1, B, N))
        self.logw = rng.normal(size=B)
        self.trans = np.array([[0.9, 0.1], [0.2, 0.8]])
        self.half = np.array([[0.9, 0.1], [0.25, 0.25]])               # row 1 sums to 0.5
        self.src_g = np.array([G, 0, 0, 0], np.int32)                  # src[0] = G is no member
        self.out = np.zeros(B * N * N)                                 # a host output large enough for every call here
        self.d = {k: torch.from_numpy(getattr(self, k)).cuda() for k in ("truth", "xi", "logw", "trans", "out")}
        torch.cuda.synchronize()

    def p(self, name):
        """the host array of that name as a pointer; "d_<name>": its device copy"""
        return self.f._p(self.d[name[2:]] if name.startswith("d_") else getattr(self, name))


# (case, entry point, arguments as a function of the Env, inside a capture, return code, must say, must not say)
TABLE = [
    ("nees_dev: NULL truth and an output in the records", "nees_dev", lambda e: (None, None, e.recs, None, None),
     False, 1, "fbus_ekf_nees_dev: truth is NULL", OVERLAP),
    ("sample_dev: NULL xi and an output in the records", "sample_dev", lambda e: (1, None, None, e.recs, None),
     False, 1, "fbus_ekf_sample_dev: xi is NULL", OVERLAP),
    ("sample: S = 0 and NULL xi", "sample", lambda e: (0, None, None, e.p("out"), None),
     False, 1, "fbus_ekf_sample: S must be", "xi is NULL"),
    ("sample_dev: S = 0, NULL xi and an output in the records", "sample_dev", lambda e: (0, None, None, e.recs, None),
     False, 1, "fbus_ekf_sample_dev: S must be", OVERLAP),
    ("group_fuse_dev: G = 3 on B = 8 and an output in the records", "group_fuse_dev",
     lambda e: (3, e.p("d_logw"), e.recs, None, None, None, None),
     False, 1, "fbus_ekf_group_fuse_dev: the batch of 8 is not a multiple of G = 3", OVERLAP),
    ("group_fuse_dev: NULL logw, the sums off, and an output in the records", "group_fuse_dev",
     lambda e: (G, None, e.recs, None, None, None, None),
     False, 1, "fbus_ekf_group_fuse_dev: logw is NULL", OVERLAP),
    ("group_fuse: NULL logw, the sums off, inside a capture", "group_fuse", lambda e: (G, None, e.p("out"), None, None, None, None),
     True, 1, "fbus_ekf_group_fuse: logw is NULL", CAPTURE),
    ("group_fuse: no output, inside a capture", "group_fuse", lambda e: (G, e.p("logw"), None, None, None, None, None),
     True, 1, "fbus_ekf_group_fuse: " + CAPTURE, None),
    ("group_collapse: src[0] = G, inside a capture", "group_collapse", lambda e: (G, e.p("src_g")),
     True, 1, "fbus_ekf_group_collapse: " + CAPTURE, "is not a member"),
    ("group_collapse: NULL src, inside a capture", "group_collapse", lambda e: (G, None),
     True, 1, "fbus_ekf_group_collapse: src is NULL", CAPTURE),
    ("group_mix: a trans row summing to 0.5, inside a capture", "group_mix", lambda e: (G, e.p("logw"), e.p("half"), None, None),
     True, 1, "fbus_ekf_group_mix: " + CAPTURE, "sums to"),
    ("group_mix: NULL logw, the sums off, inside a capture", "group_mix", lambda e: (G, None, e.p("trans"), None, None),
     True, 1, "fbus_ekf_group_mix: logw is NULL", CAPTURE),
    ("group_mix_dev: NULL trans and an output in the records", "group_mix_dev", lambda e: (G, e.p("d_logw"), None, e.recs, None),
     False, 1, "fbus_ekf_group_mix_dev: trans is NULL", OVERLAP),
    ("nees: no output, inside a capture", "nees", lambda e: (e.p("truth"), None, None, None, None),
     True, 1, "fbus_ekf_nees: " + CAPTURE, None),
    ("sample: no output, inside a capture", "sample", lambda e: (1, e.p("xi"), None, None, None),
     True, 1, "fbus_ekf_sample: " + CAPTURE, None),
    # no refusal: mix works in place, so the rule "no output asked for, nothing to do" of the calls that only read is not its rule
    ("group_mix_dev: both outputs NULL", "group_mix_dev", lambda e: (G, e.p("d_logw"), e.p("d_trans"), None, None),
     False, 0, None, None),
]


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_the_refusal_that_wins(case):
    _, entry, args, capture, want_rc, must, must_not = case
    prm, nom, rot, P, prev, _, _, _ = pose_setup(B, 32, N, 0, False)
    with make_filter(B, prm, 32, N, (nom, rot, P, prev)) as f:
        e = Env(f)
        before = f.get_state()
        lib, h = f._lib, f._h
        got = {}

        def call():
            got["rc"] = getattr(lib, "fbus_ekf_" + entry)(h, *args(e))
            got["err"] = lib.fbus_ekf_last_error(h).decode()

        if capture:
            def captured():
                # (one call that can be captured, so that the graph is not empty; it is never launched)
                f._check(lib.fbus_ekf_nees_dev(h, e.p("d_truth"), None, e.p("d_out"), None, None), "nees_dev")
                call()
            f.graph_capture(captured)
        else:
            call()
        f.sync()
        after = f.get_state()
        print(f"{entry}: rc = {got['rc']}, last error = {got['err']!r}")
        assert got["rc"] == want_rc
        same = all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(after, before))
        if want_rc == 0:
            assert not same                                     # the call ran: the records changed
        else:
            assert must in got["err"] and (must_not is None or must_not not in got["err"])
            assert same and not e.out.any() and not e.d["out"].any().item()
