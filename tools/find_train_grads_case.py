"""The search behind tests/train_step_ref.GRADS_SEED: try seeds in order until the model, images and targets of build_grads_case satisfy,
for both cases ('stats' and 'frozen'), what tests/test_train_net_host.py asserts of the chosen seed (train_step_ref.grads_case_report):
a positive prior on every pyramid level, a non-zero fp64 gradient in every trained parameter, 16 times the fp32 deviation as margin at
every ReLU above the backbone, open OHEM cuts, and the same matching in fp32 and fp64.  The search asks for SEARCH_FACTOR = 32 times the
deviation, twice what the test asserts: the fp32 oracle's rounding differs a little between hosts.  CPU only.

    python tools/find_train_grads_case.py [first [last]]          # prints one line per seed and the first that passes
"""
import os
import sys

SEARCH_FACTOR = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import train_step_ref as T
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    last = int(sys.argv[2]) if len(sys.argv) > 2 else first + 199
    for seed in range(first, last + 1):
        ok = True
        for name in T.GRADS_CASES:
            rep = T.grads_case_report(name, seed, SEARCH_FACTOR)
            print('seed %d %s: %s' % (seed, name, rep['line']), flush=True)
            if rep['failed']:
                ok = False
                break
        if ok:
            print('GRADS_SEED = %d' % seed)
            return
    raise SystemExit('no seed in %d .. %d passes' % (first, last))


if __name__ == '__main__':
    main()
