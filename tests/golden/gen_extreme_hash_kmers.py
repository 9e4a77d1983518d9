"""Generates tests/golden/extreme_hash_kmers.json: DNA k-mers whose mash hash is 0, 1, 0xFFFFFFFE or 0xFFFFFFFF.

The sketch kernels use 0xFFFFFFFF as the empty slot of their per-tile hash set and as the sort's padding, and the first
hash range starts at lo = -1, just below 0; these k-mers put genuine hashes on those edges.

The hash (src/distance.rs:21-49 and :65-87, restated by ``oracle.murmurhash3_32``) runs one murmur round per base,
h -> rotl(h ^ c(v), 13) * 5 + 0xE6546B64, then the fmix32 finaliser.  Both are invertible (5 is odd, fmix32 is a
bijection), so a meet-in-the-middle search finds preimages: the states after the first k - 12 bases of every choice of
12 bases (4^12 of them) are matched against the states reached backwards from fmix32^-1(target) through every choice of
the last 12.  About 2^16 k-mers match for each target at k >= 24; k = 32 and k = 40 fix a random prefix of k - 24
bases.  At k = 16 (8 + 8 bases) a target has a preimage with probability ~63 %; targets without one are listed as
absent.

Every k-mer stored is its own mash-canonical form (not greater than its reverse complement), so it hashes to the target
with ``canonical`` both false and true; ``revcomp`` is its reverse complement, which hashes to the target in canonical
mode only (null for a palindrome).  Where a target has no canonical preimage (k = 16 only) ``kmer`` is a preimage in
plain mode and ``canonical`` is false.  ``tests/test_oracle.py`` checks every entry against ``oracle.hash_kmer``.

    python tests/golden/gen_extreme_hash_kmers.py      (about three minutes, 1 GB of memory)
"""
import json
import pathlib

import numpy as np

OUT = pathlib.Path(__file__).with_name("extreme_hash_kmers.json")
M32 = 0xFFFFFFFF
TARGETS = (0x00000000, 0x00000001, 0xFFFFFFFE, 0xFFFFFFFF)
KS = (16, 24, 32, 40)
C1, C2 = 0xCC9E2D51, 0x1B873593


def _rotl(x, r):
    return ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


def _const(v: int) -> int:  # v * c1, rotl 15, * c2: what a base contributes to a round
    x = (v * C1) & M32
    x = ((x << 15) | (x >> 17)) & M32
    return (x * C2) & M32


CONST = np.array([_const(v) for v in range(4)], dtype=np.uint32)
INV5 = np.uint32(pow(5, -1, 1 << 32))


def _round(h, v):
    return (_rotl(h ^ CONST[v], 13) * np.uint32(5) + np.uint32(0xE6546B64)).astype(np.uint32)


def _unround(h, v):
    t = ((h - np.uint32(0xE6546B64)) * INV5).astype(np.uint32)
    return (_rotl(t, 19) ^ CONST[v]).astype(np.uint32)


def _unfmix(h: int) -> int:
    h ^= h >> 16
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & M32
    h ^= (h >> 13) ^ (h >> 26)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & M32
    h ^= h >> 16
    return h


def _expand(h0: int, nbases: int, step) -> np.ndarray:
    """states after every choice of nbases bases; index digits (base 4, most significant first) are the bases in the
    order the steps took them"""
    h = np.array([h0], dtype=np.uint32)
    v = np.arange(4)
    for _ in range(nbases):
        h = step(h[:, None], v[None, :]).ravel()
    return h


def _digits(i: int, n: int) -> list[int]:
    return [(i >> (2 * (n - 1 - j))) & 3 for j in range(n)]


def _revcomp(kmer):
    return [(b + 2) % 4 for b in reversed(kmer)]


def _is_canonical(kmer) -> bool:  # src/distance.rs:69-78: the k-mer itself is hashed unless its revcomp is smaller
    for a, b in zip(kmer, _revcomp(kmer)):
        if a != b:
            return a < b
    return True


def _hash(kmer) -> int:  # the plain (non-canonical) hash, for the self-check
    h = np.array([0x9747B28C ^ len(kmer)], dtype=np.uint32)
    for v in kmer:
        h = _round(h, v)
    x = int(h[0])
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def search(k: int, target: int, prefix: list[int]):
    """a preimage of target with the given prefix, a canonical one if any: (kmer, canonical) or None"""
    half = (k - len(prefix)) // 2
    assert len(prefix) + 2 * half == k
    h0 = np.array([0x9747B28C ^ k], dtype=np.uint32)
    for v in prefix:
        h0 = _round(h0, v)
    fwd = _expand(int(h0[0]), half, _round)                # bases prefix .. prefix + half - 1
    bwd = _expand(_unfmix(target), half, _unround)         # bases k - 1, k - 2, .. k - half
    _, fi, bi = np.intersect1d(fwd, bwd, assume_unique=False, return_indices=True)
    plain = None
    for i, j in zip(fi.tolist(), bi.tolist()):
        kmer = prefix + _digits(i, half) + _digits(j, half)[::-1]
        assert _hash(kmer) == target
        if _is_canonical(kmer):
            return kmer, True
        plain = plain or kmer
    return (plain, False) if plain else None


def main():
    rng = np.random.default_rng(20261016)
    entries, absent = [], []
    for k in KS:
        for target in TARGETS:
            prefix = rng.integers(0, 4, size=k - 24).tolist() if k > 24 else []
            found = search(k, target, prefix)
            if found is None:
                absent.append({"k": k, "target": target})
                print(f"k={k} target={target:#010x}: no preimage")
                continue
            kmer, canonical = found
            rc = _revcomp(kmer)
            entries.append({"k": k, "target": target, "kmer": "".join(map(str, kmer)), "canonical": canonical,
                            "revcomp": "".join(map(str, rc)) if canonical and rc != kmer else None})
            print(f"k={k} target={target:#010x}: {entries[-1]['kmer']} canonical={canonical}")
    OUT.write_text(json.dumps({"targets": list(TARGETS), "entries": entries, "absent": absent}, indent=1) + "\n")


if __name__ == "__main__":
    main()
