#!/usr/bin/env python3
"""Golden bits of hd_yolo_amd.optim.SGD, on an MI355X:

    python tests/golden/make_golden_optim_sgd.py          -> tests/golden/optim_sgd_bits.json

The recorded file came from the RETIRED kernel: the SGD-only `sgd_step_kernel` and its entry point, at the last commit that had them (ABI revision
14), where `SGD.step()` went through it.  tests/test_gpu_optim.py::test_sgd_bits_are_those_of_the_retired_kernel holds the surviving kernel
(`opt_step_kernel<HDY_OPT_SGD, *>` behind `hdy_opt_step`) to those bits.  This script runs whatever `SGD.step()` is today, so running it
again means ACCEPTING NEW BITS in place of the retired kernel's: do that only for a deliberate change of the update's arithmetic.

Recipe (tests/test_gpu_optim.py `sgd_bits`): `Bag()`, `make_opt(SGD, bag, **KW['SGD'])` (three groups, weight decay on the second, no
momentum in the third, Nesterov), then four times `warm_up`, `set_grads`, `step()`.  Recorded: one SHA-256 over the initial parameters, and per
step one over the gradients and one per tensor of `bag.ps` over the raw fp32 bytes of the parameter and of its momentum buffer (null where it
has none: the momentum-free group, and the late parameter before its first gradient in step 2).  The input digests tell a changed update apart
from inputs that no longer reproduce.  Before writing, the script checks that `step(ema=ema)` gives the same digests.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_gpu_optim as t  # noqa: E402


def main():
    out = os.path.join(HERE, 'optim_sgd_bits.json') if len(sys.argv) < 2 else sys.argv[1]
    bits = t.sgd_bits()
    assert t.sgd_bits(with_ema=True) == bits, 'step(ema=ema) and step() give different bits'
    with open(out, 'w') as f:
        json.dump(bits, f, indent=1)
        f.write('\n')
    print(f'wrote {out} ({os.path.getsize(out)} bytes): {len(bits["steps"])} steps, {len(bits["steps"][0]["parameters"])} tensors, '
          f'momentum buffers per step {[sum(b is not None for b in s["momentum_buffers"]) for s in bits["steps"]]}')


if __name__ == '__main__':
    main()
