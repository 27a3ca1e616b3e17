#!/usr/bin/env python3
"""Writes tests/golden/encryptor_words.json: the SHA-256 of every output of tests/encryptor_kit.py's table of cases, as THIS tree's library
gives them.  The committed file was recorded from the tree before the encryptor core (rustfhe_amd/csrc/rtfhe_encrypt.hpp) existed, with this
script and the kit copied into a checkout of that commit; re-record it only when a deterministic entry point is meant to return other words.

    python scripts/record_encryptor_words.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import encryptor_kit as ek  # noqa: E402
import rustfhe_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=ek.GOLDEN)
    args = ap.parse_args()
    words = ek.run(R)
    with open(args.out, "w") as f:
        json.dump(words, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(words), args.out))


if __name__ == "__main__":
    main()
