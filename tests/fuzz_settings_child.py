"""Child process of tests/test_fuzz_settings.py: every input of the given directory through the
front-end with the given decoder settings, framed and fed as tests/fuzz_child.py does (one
decoder per input, fed on after every rejected unit, drained at the end), under the same
address-space limit. Every event is checked against the pictures produced so far
(tests/settings_lib.check_event): none may show, read or release a picture no event produced, or
one already released. Prints one line per input; a crash or a failed check kills this process,
not the test runner.

    python fuzz_settings_child.py DIR operating_point all_layers decode_frame_type
"""
import os
import resource
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.fuzz_child import frames  # noqa: E402
from tests.settings_lib import check_event  # noqa: E402


def main(d, op, al, dft):
    if not os.environ.get("FUZZ_NO_AS_LIMIT"):
        resource.setrlimit(resource.RLIMIT_AS, (8 << 30, 8 << 30))
    from rav1d_amd.av1dec import Av1Decoder
    for name in sorted(os.listdir(d)):
        data = open(os.path.join(d, name), "rb").read()
        dec = Av1Decoder(operating_point=op, all_layers=bool(al), decode_frame_type=dft)
        have, released = set(), set()
        nev = nshow = nerr = 0

        def pump():
            nonlocal nev, nshow, nerr
            try:
                for ev in dec.events():
                    check_event(ev, have, released)
                    nev += 1
                    nshow += ev.show_pic >= 0
            except RuntimeError:
                nerr += 1

        for f in frames(data):
            try:
                dec.send(f)
            except RuntimeError:
                nerr += 1
            pump()
        dec.drain()
        pump()
        dec.drain()
        before = nev
        pump()
        assert nev == before, "a second drain queued an event"
        print(name, nev, nshow, nerr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
