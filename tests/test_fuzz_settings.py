"""The decoder settings on the reference's fuzzing corpus (tests/golden/oss_fuzz/, as
tests/test_fuzz_frontend.py runs it with the defaults): with an operating point selected, the
lower spatial layers held back and every decode_frame_type, each input must end in events or
-errno returns. No crash, and no event that shows, reads or releases a picture that no event
produced (a slot left without a picture by a skipped frame must be an error, not an event). The
whole corpus runs in about a second per setting, so none of it is left out."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = os.path.join(HERE, "golden", "oss_fuzz")

# (operating_point, all_layers, decode_frame_type)
SETTINGS = [(1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 0, 3), (0, 1, 1), (0, 1, 2), (0, 1, 3)]


@pytest.mark.parametrize("op,al,dft", SETTINGS, ids=[f"op{o}-al{a}-dft{d}" for o, a, d in SETTINGS])
def test_fuzz_corpus_with_settings(op, al, dft):
    names = sorted(os.listdir(CORPUS))
    assert len(names) >= 100
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_settings_child.py"), CORPUS, str(op), str(al), str(dft)],
                       capture_output=True, text=True, timeout=600)
    done = [ln.split()[0] for ln in r.stdout.splitlines() if ln.strip()]
    assert r.returncode == 0, f"front-end died or an event failed its check (rc {r.returncode}) after {done[-1:]}: {r.stderr[-800:]}"
    assert done == names
