# variant: stream priorities - the chunk pipelines' own main streams (camera,
# closest-hit walk, classify, shade: the critical path; slot 0's is the
# caller's stream) created at the greatest priority (SIDE=1: every slot's
# side stream instead)
import os, sys
p = sys.argv[1] + "/pt_kernels.hip"
s = open(p).read()
which = "b.side" if os.environ.get("SIDE") == "1" else "b.main"
a = "PTG_HIP(hipStreamCreateWithFlags(&%s, hipStreamNonBlocking));" % which
assert s.count(a) == 1
s = s.replace(a, """{
            int least = 0, greatest = 0;
            PTG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
            PTG_HIP(hipStreamCreateWithPriority(&%s, hipStreamNonBlocking, greatest));
        }""" % which)
open(p, "w").write(s)
