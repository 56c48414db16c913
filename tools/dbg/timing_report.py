import numpy as np, sys
a=np.loadtxt(sys.argv[1], dtype=np.uint64).astype(np.int64)
t0=a[:,0].min()
rel=(a[:,:5]-t0)*10.0/1000.0   # 100 MHz ticks -> us
print("blocks", len(a))
names=["start","after head","after counts","after loop","end"]
for i,n in enumerate(names):
    print("%-14s min %.2f  median %.2f  p90 %.2f  max %.2f us  (spread %.2f)"%(n, rel[:,i].min(), np.median(rel[:,i]), np.percentile(rel[:,i],90), rel[:,i].max(), rel[:,i].max()-rel[:,i].min()))
d=np.diff(rel,axis=1)
for i,n in enumerate(["head","counts","loop","tail"]):
    print("phase %-8s median %.2f  p90 %.2f  max %.2f us"%(n, np.median(d[:,i]), np.percentile(d[:,i],90), d[:,i].max()))
print("outputs per block: min %d median %d max %d"%(a[:,5].min(), np.median(a[:,5]), a[:,5].max()))
# where each block ran (DEVTOOLS builds: column 6 = HW_REG_HW_ID, column 7 = HW_REG_XCC_ID): the stagger of the blocks that shared a CU
if a.shape[1] >= 8 and a[:,6].any():
    hw, xcc = a[:,6], a[:,7] & 0xf
    cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xf)     # xcc, se_id, sh_id, cu_id
    ids, inv, cnt = np.unique(cu, return_inverse=True, return_counts=True)
    print("CUs %d; blocks per CU: %s"%(len(ids), ", ".join("%d CUs hold %d"%((cnt==k).sum(), k) for k in sorted(set(cnt)))))
    rows = {"loop entry": 2, "loop exit": 3, "end": 4}
    for k in sorted(set(cnt)):
        if k < 2: continue
        sel = [np.where(inv == i)[0] for i in np.where(cnt == k)[0]]
        for n, c in rows.items():
            first = np.array([rel[s, c].min() for s in sel]); last = np.array([rel[s, c].max() for s in sel])
            print("CUs of %d blocks, %-10s first of the CU: median %.2f max %.2f   last of the CU: median %.2f max %.2f   stagger (last - first): median %.2f  p90 %.2f  max %.2f us"%(
                k, n, np.median(first), first.max(), np.median(last), last.max(), np.median(last-first), np.percentile(last-first,90), (last-first).max()))
        # the blocks of a CU in the order they entered the loop: how long each stayed in it
        order = np.array([d[s, 2][np.argsort(rel[s, 2])] for s in sel])
        print("CUs of %d blocks, loop time by order of entry on the CU: %s us (medians)"%(k, "  ".join("%.2f"%v for v in np.median(order, axis=0))))
