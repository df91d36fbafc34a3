# variant: the exact (MathExact) shading pass capped at 64 VGPRs (8 waves per SIMD), so its
# few waves find room beside the persistent certified kernels
import sys
p = sys.argv[1] + "/pt_kernels.hip"
s = open(p).read()
a = "amdgpu_waves_per_eu(MP::kFast ? PTG_SHADE_WAVES : 2, 8)"
assert a in s, a
open(p, "w").write(s.replace(a, "amdgpu_waves_per_eu(MP::kFast ? PTG_SHADE_WAVES : 8, 8)"))
