"""The planner's decisions, held to a committed fingerprint (host only: no GPU).

tools/plan_fingerprint.py walks every network x batch size x geometry x plan option and the per-op scratch / slice queries over a
grid of shapes and ABI tile numbers; tests/golden/plan_fingerprint.json holds the SHA-256 of every case's record (its
"generated_from" names the commit whose library wrote it).  The built library must reproduce every digest: the launch lists, side
streams, workspace sizes, flops, derived-buffer sizes, taps, training workspace sizes, refusal texts and query results are integers
and strings computed by fixed formulas, so there is no tolerance.  A change that moves a kernel choice on purpose regenerates the
fixture (plan_fingerprint.py --golden) and the fixture's diff names the cases that moved."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import plan_fingerprint as F      # noqa: E402


def test_built_library_reproduces_the_plan_fingerprint():
    with open(F.GOLDEN) as f:
        want = json.load(f)['cases']
    seen = []
    for cid, rec in F.cases():
        seen.append(cid)
        if want.get(cid) != F.digest(rec):
            print('first differing case: %s\nexpected [sha256, size] %s, got %s\nrecord of the built library:\n%s'
                  % (cid, want.get(cid), F.digest(rec), json.dumps(rec, sort_keys=True, indent=1)))
            assert want.get(cid) == F.digest(rec), 'plan fingerprint differs at %s (full record printed above)' % cid
    assert seen == list(want), 'the case list differs from the fixture: %d cases here, %d there' % (len(seen), len(want))
