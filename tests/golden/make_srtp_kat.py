"""Writes tests/golden/srtp_kat.json: known answers for tests/srtp_model.py from the openssl command line, data only.
  ecb    `openssl enc -aes-128-ecb -nopad` over single blocks and runs of blocks, seeded keys;
  ctr    `openssl enc -aes-128-ctr` keystreams (the encryption of zeros) for seeded keys and IVs, among them counters that
         carry from byte 15 into byte 14 -- never beyond it, so that the 16-bit counter of SRTP and openssl's 128-bit one
         agree;
  hmac   `openssl dgst -sha1 -mac HMAC -macopt hexkey:` tags over seeded messages of every length 0..200, 20-byte keys.
Run it from anywhere: python tests/golden/make_srtp_kat.py [OUT]"""
import json
import random
import shutil
import subprocess
import sys
from pathlib import Path


def _openssl(args, data):
    r = subprocess.run([shutil.which("openssl")] + args, input=data, capture_output=True, timeout=60)
    if r.returncode != 0:
        raise RuntimeError("openssl %s: %s" % (" ".join(args), r.stderr.decode(errors="replace")))
    return r.stdout


def make():
    rnd = random.Random(37110)
    rb = lambda n: bytes(rnd.randrange(256) for _ in range(n))  # noqa: E731
    ecb = []
    for nblocks in [1] * 16 + [2, 3, 17, 64]:
        key, data = rb(16), rb(16 * nblocks)
        out = _openssl(["enc", "-aes-128-ecb", "-nopad", "-K", key.hex()], data)
        ecb.append({"key": key.hex(), "in": data.hex(), "out": out.hex()})
    ctr = []
    lens = [1, 15, 16, 17, 31, 32, 33, 47, 48, 100, 255, 256, 1388, 4096]
    for k in range(36):
        key, iv, n = rb(16), bytearray(rb(16)), lens[k % len(lens)]
        nb = (n + 15) // 16
        if k % 3 == 0:  # byte 15 carries into byte 14 inside the run
            iv[14] = rnd.randrange(0, 255)
            iv[15] = 256 - rnd.randrange(1, nb) if nb > 1 else 255
        elif k % 3 == 1:  # the SRTP form: the last two bytes start at 0
            iv[14] = iv[15] = 0
        else:  # anywhere, as long as the 16 bits do not wrap
            c = rnd.randrange(0, 65536 - nb)
            iv[14], iv[15] = c >> 8, c & 255
        assert int.from_bytes(iv[14:], "big") + nb <= 65536
        out = _openssl(["enc", "-aes-128-ctr", "-K", key.hex(), "-iv", bytes(iv).hex()], bytes(n))
        ctr.append({"key": key.hex(), "iv": bytes(iv).hex(), "n": n, "out": out.hex()})
    mac = []
    for n in range(201):
        key, msg = rb(20), rb(n)
        out = _openssl(["dgst", "-sha1", "-mac", "HMAC", "-macopt", "hexkey:" + key.hex(), "-binary"], msg)
        mac.append({"key": key.hex(), "msg": msg.hex(), "out": out.hex()})
    return {"ecb": ecb, "ctr": ctr, "hmac": mac}


def dumps(rec):
    return json.dumps(rec, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).resolve().parent / "srtp_kat.json"
    out.write_text(dumps(make()))
