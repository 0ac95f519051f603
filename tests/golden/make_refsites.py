"""Record SHA-256 digests of the reference's TensorFlow call-site lines into a fixture.

Run where a checkout of the reference (lizaibeim/mmla-audio) exists:
    python tests/golden/make_refsites.py <path/to/reference>
-> tests/golden/refsites_sha256.json: for every entry of tests/refsites.py (file, first line, number
of lines) the digest of the reference's own lines at that place, each stripped of surrounding white
space and joined with '\\n'.  The fixture holds digests only, no source text;
tests/test_tf_compat_cpu.py::test_call_site_text_matches_reference compares the digest of the text
in tests/refsites.py against it, so the check needs no reference checkout.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refsites  # noqa: E402

OUT = os.path.join(HERE, 'refsites_sha256.json')


def digest(lines):
    return hashlib.sha256('\n'.join(l.strip() for l in lines).encode('utf-8')).hexdigest()


def main(ref):
    out = []
    for path, line, text in refsites.ALL:
        n = len(text.rstrip('\n').split('\n'))
        lines = open(os.path.join(ref, path)).read().split('\n')
        out.append({'file': path, 'line': line, 'lines': n, 'sha256': digest(lines[line - 1:line - 1 + n])})
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])
