"""Compare two `bench.py --dump-outputs DIR` directories array by array, byte for byte (CPU only): python tools/cmp_dumps.py DIR_A DIR_B
Used for A/B records (profiles/r17): one dump with MORB_HIP_LIB naming the parent's library, one with the new build.  Exit status 1 if any
array differs or the two directories do not hold the same files."""
import os, sys
import numpy as np
a, b = sys.argv[1], sys.argv[2]
names = sorted(os.listdir(a)); diff = 0
for n in names:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    diff += not same
    print(f"{n:40s} {str(x.shape):20s} {str(x.dtype)} {'identical' if same else 'DIFFERENT'}")
print("arrays", len(names), "different", diff)
sys.exit(1 if diff or sorted(os.listdir(b)) != names else 0)
