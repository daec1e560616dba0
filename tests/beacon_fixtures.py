"""The random beacon restated in plain Python for the tests (include/graph_witness_groth16_beacon.h): the hash chain and the
derivation with hashlib, and the expected beacon record of either phase from the contribution fixtures."""
import hashlib
import struct

from tests import ceremony_fixtures as CE
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF

R = GF.R


def chain(beacon_hash, iterations_exp):
    d = bytes(beacon_hash)
    for _ in range(1 << iterations_exp):
        d = hashlib.sha256(d).digest()
    return d


def scalars(phase, beacon_hash, iterations_exp):
    """phase 1: [tau', alpha', beta', s_0, s_1, s_2]; phase 2: [delta', s]"""
    d, out = chain(beacon_hash, iterations_exp), []
    for j in range(6 if phase == 1 else 2):
        ctr = 0
        while True:
            x = int.from_bytes(hashlib.blake2b(b"cwc-beacon" + bytes([phase]) + d + bytes([j]) + struct.pack("<I", ctr)).digest(), "big") % R
            ctr += 1
            if x:
                out.append(x)
                break
    return out


def as_beacon(rec, name, iterations_exp, beacon_hash):
    """a fixture's contribution record (of either phase) marked as a beacon: type 1 and the beacon's parameters"""
    rec.type, rec.params = 1, CF.beacon_params(name, iterations_exp, bytes(beacon_hash))
    return rec


def ptau_beacon_record(challenge, logs, beacon_hash, iterations_exp, name=""):
    """the record ptau_beacon appends to a file whose logs are `logs`, after the challenge `challenge`"""
    x = scalars(1, beacon_hash, iterations_exp)
    return as_beacon(CE.contribution(challenge, logs, tuple(x[:3]), tuple(x[3:]), name), name, iterations_exp, beacon_hash)


def zkey_beacon_record(cs_hash, before, delta_prev, beacon_hash, iterations_exp, name=""):
    """the record groth16_beacon appends after `before`, delta_prev the key's delta1 (affine)"""
    delta, s = scalars(2, beacon_hash, iterations_exp)
    return as_beacon(CF.contribution(cs_hash, before, delta_prev, delta, s, name), name, iterations_exp, beacon_hash)
