"""Writes tests/golden/leg_paths_pinned.npz: what fcpp_debug_field_paths and fcpp_debug_headland_paths of THIS tree return for the 28 cases
of tests/test_leg_paths_pinned.py (which says what is stored, and how it is compared).  Run on the commit whose behaviour is to be pinned,
on the CPU, after the library is built:
    python tools/record_leg_paths.py --commit $(git rev-parse HEAD)
The commit is stored under 'commit'.  --out writes elsewhere (to compare two trees' recordings file against file)."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import test_leg_paths_pinned as P          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the 40 hex digits of the commit this tree is')
    ap.add_argument('--out', default=P.GOLDEN)
    args = ap.parse_args()
    if len(args.commit) != 40 or set(args.commit) - set('0123456789abcdef'):
        raise SystemExit('--commit takes a full commit hash')
    rec = {'commit': np.array(args.commit)}
    for name, (cut, kw) in P.field_cases().items():
        rec.update(P.recording(name, P.host_field_case(cut, kw), P.FIELD_FULL + P.FIELD_HOST_FULL, P.DIGESTS + P.HOST_DIGESTS))
    for name, (rg, kw) in P.headland_cases().items():
        rec.update(P.recording(name, P.host_headland_case(rg, kw), P.RING_FULL + P.RING_HOST_FULL, P.DIGESTS + P.HOST_DIGESTS))
    np.savez_compressed(args.out, **rec)
    print('%s: %d arrays, %d bytes' % (args.out, len(rec), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
