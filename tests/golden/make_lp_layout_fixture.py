"""Records lp_layout_parent.npz: the storage layout of the batched LP kernels, table for table, for the cases below.

    python tests/golden/make_lp_layout_fixture.py [LIBRARY [OUT.npz]]

LIBRARY is the liblpbox_hip.so to record from (default: the one built in the tree).  The committed file was recorded from the commit
BEFORE the layout planner was split out of lpbox_capi.hip (csrc/lpbox_lp_layout.cpp): that library, built with a scratch patch that
kept the host vectors of its finalize() and served them through lpbox_debug_get_lp_table, run on a machine with a GPU (it planned
only behind its device check).  The library of the tree must reproduce the file exactly, on any machine:
tests/test_lp_layout.py::test_layout_equals_the_recorded_one calls record() below and compares every array.

The file: many of the arrays are equal across cases (a knob that moves row tasks leaves the column tables alone), the pointer tables are
monotone, and a zip member costs more than a small array, so pack() stores every distinct array once, the pointer tables as
differences, all of one integer type in one member ("u1", "u2", "i4"), and "index" = the JSON of name -> (member, offset, shape,
1 = differences); load() undoes it.

Keys: "<case>/<instance>/<what>", what = layout, row_split, col_split_own, col_split_help, the nine tables of lpbox_debug_get_lp_table
at the strides of the batch, wave_classes where the geometry is 512 x 1 in the default order, and "<case>/config" =
(threads, slots per thread, LDS bytes, 1 = specialised PCG loop).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "accelerated-lpbox-admm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "lp_layout_parent.npz")
TABLES = ("rs_ptr", "rs_col", "cs_ptr", "cs_row", "hs_ptr", "rid", "rgl", "rmeta", "cmeta")
KNOBS = ("THREADS", "NOSORT", "NOSPLIT", "BANKAWARE", "NOCONFLICT", "SNAKEROWS", "NOCOLSPLIT", "SPLITBIAS", "SNAKECOLS", "PCGLOOP", "REF_VALS")


def _file_instance(k, j):
    """instance/<k>_<j>/instance_1_{C,b}.txt: valued instances (k == 2 negates the values), so they go to the reference order."""
    from lpbox_hip.lp import LpBatch
    b = LpBatch(batch=1, order="reference")
    b.read_file(0, 1, k, j, root=HERE)
    return b.get_problem(0)


def _instances(name, count):
    """The first `count` instances of an lp_*.npz fixture (what oracle.load_lp_batch returns, with every array of the file read once)."""
    d = dict(np.load(os.path.join(HERE, name)))
    out, cp, ri, pr = [], 0, 0, 0
    for n, l, nnz in list(zip(d["n"], d["l"], d["nnz"]))[:count]:
        n, l, nnz = int(n), int(l), int(nnz)
        out.append(dict(n=n, l=l, colptr=d["colptr"][cp:cp + n + 1].astype(np.int32), rowidx=d["rowidx"][ri:ri + nnz].astype(np.int32),
                        b=-1.0 * d["price"][pr:pr + n]))
        cp += n + 1; ri += nnz; pr += n
    return out


def _valued(I):
    """The same pattern with stored values other than 1 (what they are does not enter the layout, only where the kernels keep them)."""
    J = dict(I)
    J["vals"] = 0.5 + 0.25 * (np.arange(len(I["rowidx"])) % 5)
    return J


def cases():
    """(name, environment, order, instances)"""
    small, mid, large = _instances("lp_20_60_seed0.npz", 3), _instances("lp_100_500_seed0.npz", 1)[0], _instances("lp_500_2000_seed0.npz", 1)[0]
    out = [("instance_2_7", {}, "reference", [_file_instance(2, 7)]), ("instance_3_7", {}, "reference", [_file_instance(3, 7)]),
           ("lp_20_60_0", {}, "default", [small[0]]), ("lp_20_60_2", {}, "default", [small[2]]),
           ("lp_100_500", {}, "default", [mid]), ("lp_500_2000", {}, "default", [large])]
    for knob, val in (("THREADS", "256"), ("THREADS", "1024"), ("BANKAWARE", "1"), ("NOSORT", "1"), ("NOSPLIT", "1"), ("NOCOLSPLIT", "1"),
                      ("SPLITBIAS", "0")):
        out.append(("lp_100_500_%s_%s" % (knob.lower(), val), {"LPBOX_LP_" + knob: val}, "default", [mid]))
    out.append(("lp_100_500_reference", {}, "reference", [mid]))
    out.append(("lp_100_500_reference_valued", {}, "reference", [_valued(mid)]))
    for knob, val in (("BANKAWARE", "0"), ("SNAKEROWS", "1"), ("SNAKECOLS", "1")):
        out.append(("lp_500_2000_%s_%s" % (knob.lower(), val), {"LPBOX_LP_" + knob: val}, "default", [large]))
    out.append(("batch_20_60_and_100_500", {}, "default", [small[0], mid]))
    return out


def narrow(a):
    """The narrowest integer type that holds every value."""
    a = np.asarray(a)
    for t in (np.uint8, np.uint16, np.int32):
        if a.size == 0 or (a.min() >= np.iinfo(t).min and a.max() <= np.iinfo(t).max):
            return a.astype(t)
    return a


def record():
    """name -> array for every case, from the library lpbox_hip loads.  The LPBOX_LP_* environment is set per case and put back."""
    from lpbox_hip.lp import LpBatch
    saved = {k: os.environ.pop("LPBOX_LP_" + k, None) for k in KNOBS}
    got = {}
    try:
        for name, env, order, insts in cases():
            os.environ.update(env)
            try:
                b = LpBatch(insts, order=order)
                cfg = b.config()                # the layout is planned, with the environment read, here
            finally:
                for k in env:
                    del os.environ[k]
            got[name + "/config"] = narrow([cfg["threads"], cfg["elems_per_thread"], cfg["lds_bytes"], int(cfg["pcg_loop"] == "specialised")])
            for i in range(len(insts)):
                own, help4 = b.col_split(i)
                arrs = dict(layout=b.layout(i), row_split=b.row_split(i), col_split_own=own, col_split_help=help4)
                arrs.update((t, b.debug_table(t, i)) for t in TABLES)
                if order == "default" and (cfg["threads"], cfg["elems_per_thread"]) == (512, 1):
                    arrs["wave_classes"] = b.wave_classes(i)
                for k, v in arrs.items():
                    got["%s/%d/%s" % (name, i, k)] = narrow(v)
            b.close()
    finally:
        os.environ.update({"LPBOX_LP_" + k: v for k, v in saved.items() if v is not None})
    return got


def pack(got):
    """name -> array, as record() returns it  ->  the members of the file (see the module's docstring)."""
    pools, index, seen = {}, {}, {}
    for k in sorted(got):
        diff = k.endswith("_ptr")
        v = narrow(np.diff(got[k].astype(np.int64), prepend=0)) if diff else got[k]
        ident = (v.dtype.str, v.shape, int(diff), v.tobytes())
        if ident not in seen:
            member = "%s%d" % (v.dtype.kind, v.dtype.itemsize)
            seen[ident] = (member, sum(len(a) for a in pools.setdefault(member, [])))
            pools[member].append(v.ravel())
        index[k] = [*seen[ident], list(v.shape), int(diff)]
    out = {m: np.concatenate(a) for m, a in pools.items()}
    out["index"] = np.frombuffer(json.dumps(index, sort_keys=True).encode(), np.uint8)
    return out


def load(path=OUT):
    """The file -> name -> array, each as record() returns it."""
    d = dict(np.load(path))
    got = {}
    for k, (member, off, shape, diff) in json.loads(d["index"].tobytes().decode()).items():
        v = d[member][off:off + int(np.prod(shape))].reshape(shape)
        got[k] = narrow(np.cumsum(v.astype(np.int64))) if diff else v
    return got


if __name__ == "__main__":
    if len(sys.argv) > 1:
        from lpbox_hip import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    got = record()
    np.savez_compressed(out, **pack(got))
    print("%s: %d arrays, %d bytes" % (out, len(got), os.path.getsize(out)))
