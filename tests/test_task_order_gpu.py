"""The encoders do not care where a task stands inside its bin of the sorted task list. The sort (search_common.h) promises sizes that do not rise
along the list; the positions inside a bin come from LDS and global atomics, and which wavefront takes which batch of the queue is decided the same
way, so the suite only ever sees the orders this hardware tends to produce. The development build's DXTEX_TASK_ORDER_REVERSE reverses every bin in
place after the scatter, in both encoders: another order the atomics could have produced. The payloads must be the ones of the plain run, byte for
byte, and the ones the suite pins for these inputs (the corpus golden files, the reference encoder for the dedupe test's base image).

The inputs are images other tests already compress: the image-form cases of tests/test_bc7_corpus_gpu.py at flags 0 and BC7_USE_3SUBSETS, the 64 x 64
base image of tests/test_bc7_block_dedupe_gpu.py at flags 0, BC7_USE_3SUBSETS and BC7_QUICK, and the smooth images of tests/test_bc6h_corpus_gpu.py
at both formats. Three processes on the development build: plain, reversed, and reversed with 64 blocks a pass so that short lists are reversed too.
Under DXTEX_BC7_STATS a reversing sort prints `task order: reversed N bins`, N the bins that held two tasks or more."""
import functools
import hashlib
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bc6h_corpus as C6  # noqa: E402
import bc7_corpus as C7  # noqa: E402

pytestmark = pytest.mark.gpu
BC7, RGBA8, UF16, SF16, RGBA16F = 98, 28, 95, 96, 10
USE_3SUBSETS, QUICK = 0x80000, 0x100000
GOLDEN7 = {0: os.path.join(ROOT, "tests", "golden", "bc7_corpus_default.npz"), USE_3SUBSETS: os.path.join(ROOT, "tests", "golden", "bc7_corpus_3subsets.npz")}
GOLDEN6 = {UF16: os.path.join(ROOT, "tests", "golden", "bc6h_corpus_uf16.npz"), SF16: os.path.join(ROOT, "tests", "golden", "bc6h_corpus_sf16.npz")}
CROP_SET = {0: "two_alpha", USE_3SUBSETS: "three_opaque"}          # as tests/test_bc7_corpus_gpu.py crops them


@functools.lru_cache(maxsize=None)
def _cases():
    """[(name, image, width, height, source format, target format, flags)], every image read-only."""
    import test_bc7_block_dedupe_gpu as D
    t7, t6 = C7.corpus(), C6.corpus()
    out = []
    images = {name: C7.as_image(t7[name]) for name in ("two_opaque", "two_alpha", "three_opaque")}
    images["mixed"] = C7.as_image(np.concatenate([t7[s] for s in C7.MIXED_SETS]))
    for name, (img, w, h) in images.items():
        for flags in (0, USE_3SUBSETS):
            out.append((f"bc7-{name}", img, w, h, RGBA8, BC7, flags))
    for flags, name in CROP_SET.items():
        for i, crop in enumerate(C7.crops(t7[name])):
            out.append((f"bc7-crop{i}-{name}", crop, C7.CROP_W, C7.CROP_H, RGBA8, BC7, flags))
    for flags in (0, USE_3SUBSETS, QUICK):
        out.append(("bc7-dedupe-base", D._base_image(), 64, 64, RGBA8, BC7, flags))
    for name in ("smooth", "smooth_signs"):
        img, w, h = C6.as_image(t6[name])
        for fmt in (UF16, SF16):
            out.append((f"bc6h-{name}", img.astype(np.float16), w, h, RGBA16F, fmt, 0))
    for c in out:
        c[1].setflags(write=False)
    assert len({(c[0], c[5], c[6]) for c in out}) == len(out)
    return tuple(out)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _dev_run(env_items):
    """Every case through the development build in one process of its own. Per payload a line `payload NAME FORMAT FLAGS SHA256`, preceded by
    the `task order` lines of its sorts. Returns {(name, format, flags): (sha, [N of every reversing sort])}."""
    code = textwrap.dedent("""
        import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)
        import directxtex_amd as dx
        import test_task_order_gpu as t
        dx.capi.load(dev=True)          # only the -DDXTEX_DEV build reads knobs
        c = dx.Context(0)
        for name, img, w, h, src, dst, flags in t._cases():
            payload = c.compress(img, w, h, src, dst, flags, 0.5)
            sys.stderr.flush()
            print("payload", name, dst, hex(flags), t._sha(payload), flush=True)
        c.close()
    """ % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DXTEX_BC7_STATS="1", **dict(env_items)), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    out, bins = {}, []
    for line in r.stdout.splitlines():
        m = re.match(r"task order: reversed (\d+) bins", line)
        if m:
            bins.append(int(m.group(1)))
        elif line.startswith("payload "):
            _, name, fmt, flags, sha = line.split()
            out[(name, int(fmt), int(flags, 16))] = (sha, bins)
            bins = []
    assert len(out) == len(_cases()), r.stdout[-3000:]
    return out


def _run(**env):
    return _dev_run(tuple(sorted(env.items())))


def _shas(run):
    return {k: v[0] for k, v in run.items()}


def _differing(a, b):
    return sorted(k for k in a if a[k] != b[k])


@functools.lru_cache(maxsize=None)
def _pinned():
    """{(name, format, flags): sha} of what the corpus golden files hold for the cases they cover."""
    want = {}
    g7 = {flags: dict(np.load(path)) for flags, path in GOLDEN7.items()}
    g6 = {fmt: dict(np.load(path)) for fmt, path in GOLDEN6.items()}
    for name, img, w, h, src, dst, flags in _cases():
        nblocks = ((w + 3) // 4) * ((h + 3) // 4)
        kind = name.split("-", 1)[1]
        if dst == BC7 and kind == "mixed" and flags == 0:
            want[name, dst, flags] = _sha(C7.image_payload(np.concatenate([g7[0][s] for s in C7.MIXED_SETS]), nblocks))
        elif dst == BC7 and kind in g7.get(flags, {}) and kind != "crops":
            want[name, dst, flags] = _sha(C7.image_payload(g7[flags][kind], nblocks))
        elif dst == BC7 and kind.startswith("crop"):
            want[name, dst, flags] = _sha(g7[flags]["crops"][int(kind[4:].split("-")[0])])
        elif dst in g6 and kind in g6[dst]:
            want[name, dst, flags] = _sha(g6[dst][kind])
    return want


def test_the_golden_files_pin_the_cases_the_corpus_tests_compress():
    pinned = set(_pinned())
    assert {("bc7-mixed", BC7, 0), ("bc7-two_opaque", BC7, 0), ("bc7-two_alpha", BC7, 0), ("bc7-three_opaque", BC7, USE_3SUBSETS),
            ("bc6h-smooth", UF16, 0), ("bc6h-smooth", SF16, 0), ("bc6h-smooth_signs", SF16, 0)} <= pinned
    assert sum(1 for k in pinned if k[0].startswith("bc7-crop")) == 16
    assert ("bc7-two_opaque", BC7, USE_3SUBSETS) not in pinned and ("bc6h-smooth_signs", UF16, 0) not in pinned


def test_plain_run_gives_the_pinned_payloads(oracle):
    import test_bc7_block_dedupe_gpu as D
    plain = _run()
    assert all(v[1] == [] for v in plain.values()), "a sort reversed its bins without the knob"
    got = _shas(plain)
    bad = sorted(k for k, sha in _pinned().items() if got[k] != sha)
    assert not bad, f"the development build without the knob misses the golden payloads of {bad}"
    for flags in (0, USE_3SUBSETS, QUICK):
        assert got["bc7-dedupe-base", BC7, flags] == _sha(oracle.ref_compress_image(D._base_image(), 64, 64, RGBA8, BC7, flags, 0.5)), hex(flags)


def _knob_did_something(run):
    for prefix in ("bc7-", "bc6h-"):
        assert any(n > 0 for k, v in run.items() if k[0].startswith(prefix) for n in v[1]), f"no {prefix} sort reversed a bin of two tasks or more"
    assert all(v[1] for v in run.values()), "a payload was made without a reversing sort"


def test_reversed_bins_give_the_same_payloads():
    plain, rev = _run(), _run(DXTEX_TASK_ORDER_REVERSE="1")
    _knob_did_something(rev)
    bad = _differing(_shas(plain), _shas(rev))
    assert not bad, f"payloads change with the order inside the bins: {bad}"
    assert not [k for k, sha in _pinned().items() if rev[k][0] != sha]


def test_reversed_bins_of_short_lists_give_the_same_payloads():
    """64 blocks a pass: lists of a few hundred tasks, the lengths at which the group-of-lanes kernels and one-task-per-lane batches work."""
    plain, rev = _run(), _run(DXTEX_TASK_ORDER_REVERSE="1", DXTEX_MAX_BLOCKS_PER_PASS="64")
    _knob_did_something(rev)
    bad = _differing(_shas(plain), _shas(rev))
    assert not bad, f"payloads change with the order inside the bins at 64 blocks a pass: {bad}"
    assert not [k for k, sha in _pinned().items() if rev[k][0] != sha]
