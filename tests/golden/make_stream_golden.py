"""Generates tests/golden/stream_golden.json: the bytes the REFERENCE's own src/utils/stream_helper.py (write_sps /
write_ip) writes for tests/test_stream_native.py::_sequence(), as length + sha256 (run in the build container, where
/root/reference exists).

Usage: python tests/golden/make_stream_golden.py
"""
import hashlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from test_stream_native import _python_bytes, _sequence  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("ref_stream_helper", "/root/reference/src/utils/stream_helper.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    data = _python_bytes(_sequence(), ref)
    out = {"source": "src/utils/stream_helper.py write_sps / write_ip of the reference, units of test_stream_native._sequence()",
           "bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
    with open(os.path.join(HERE, "stream_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
