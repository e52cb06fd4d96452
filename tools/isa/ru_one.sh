#!/bin/bash
# resource usage of ONE object of the library (default: the register-state pair kernel), compiled as the product compiles it
# (poreover_amd/build.py --cmd): tools/isa/ru_one.sh [OBJECT] [extra hipcc flags]     OBJECT: po_pair, po_beam2d_reg_wide.hip, ...
# po_beam2d_reg is the library's object of that name, i.e. the 32-slot kernels only (the 64-slot ones: po_beam2d_reg_wide); all
# fifteen instantiations in one listing, as this script gave before it took the product's options: po_beam2d_reg -UPO_REG_TU
f=$(basename ${1:-po_beam2d_reg.hip}); shift
cd $(dirname $0)/../..
eval "$(python3 poreover_amd/build.py --cmd $f "$@") -S --cuda-device-only -o /tmp/ru_one.s" 2>/dev/null
python3 - <<'PY'
import re,subprocess
txt=open('/tmp/ru_one.s').read()
meta=txt[txt.index("amdhsa.kernels:"):]
for blk in meta.split("  - .agpr_count:")[1:]:
    g=lambda k:(re.search(r"\.%s:\s+(\S+)"%k,blk) or [None,"0"])[1]
    dem=subprocess.run(["c++filt",g("name")],capture_output=True,text=True).stdout.strip()
    dem=re.sub(r"\(.*","",dem).replace("void ","").replace("(anonymous namespace)::","")
    print("%-45s vgpr %s sgpr %s sgpr_spill %s vgpr_spill %s scratch %s lds %s"%(dem,g("vgpr_count"),g("sgpr_count"),g("sgpr_spill_count"),g("vgpr_spill_count"),g("private_segment_fixed_size"),g("group_segment_fixed_size")))
PY
