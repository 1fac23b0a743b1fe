"""A sequential numpy restatement of the six fit kernels of csrc/gbt.hip, for the CPU suite: the same row keys, per-level segment tables,
stable partition with the kernel's destination rule (asserted to hit every slot once), level-order node numbering, stop rules and tie
rule (lowest feature, then lowest position, among equal computed scores).  Its sums run in numpy's order, not the kernels', so its trees
need not equal the GPU's bit for bit; like any fit it is judged by tests/gbt_replay.py.  ``fit`` returns (trees, init, raw scores after
every stage [T, n], train scores [T])."""
import numpy as np
from scipy.special import logit


def resid(y,raw):
    e=np.exp(-raw); return -(((1-y)-y*e)/(1+e))
def fit(X,y,T,lr,D,mss,msl):
    X32=np.ascontiguousarray(X,dtype=np.float32); n,d=X32.shape; XT=X32.T.copy()
    order0=np.argsort(XT,axis=1,kind='stable').astype(np.int32)
    eps=np.finfo(np.float32).eps; init=float(logit(np.clip(y.mean(),eps,1-eps)))
    raw=np.full(n,init); g=resid(y,raw)
    cap=(2<<D)-1
    out=dict(left=[],right=[],feature=[],threshold=[],value=[],n_node_samples=[],root=[0]); ts=[]; stages=[]
    for t in range(T):
        left=np.full(cap,-9);right=np.full(cap,-9);feat=np.zeros(cap,int);thr=np.zeros(cap);val=np.zeros(cap);nns=np.zeros(cap,int)
        key=np.zeros(n,int); order=order0.copy(); n_nodes=1
        tab=dict(start=[0],cnt=[n],node=[0],flag=[1],sg=[0.0],spq=[0.0]); level=0
        while True:
            nk=1<<level; active=0
            for k in range(nk):
                if tab['flag'][k]!=1: continue
                s,m=tab['start'][k],tab['cnt'][k]; rows=order[0][s:s+m]
                sg=g[rows].sum(); sq=(g[rows]**2).sum(); pr=y[rows]-g[rows]; spq=(pr*(1-pr)).sum()
                mean=sg/m; imp=sq/m-mean*mean
                leaf= level>=D or m<mss or m<2*msl or imp<=2.220446049250313e-16
                node=tab['node'][k]; tab['sg'][k]=sg; tab['spq'][k]=spq; nns[node]=m
                if leaf:
                    tab['flag'][k]=2; left[node]=right[node]=-1; thr[node]=-2.0
                    den=spq/m; val[node]=0.0 if abs(den)<1e-150 else (sg/m)/den
                else: val[node]=mean; active+=1
            if active==0: break
            # split
            cand={}
            for f in range(d):
                o=order[f]; kk=key[o]
                for k in range(nk):
                    if tab['flag'][k]!=1: continue
                    s,m=tab['start'][k],tab['cnt'][k]
                    assert (kk[s:s+m]==k).all()
                    rows=o[s:s+m]; fv=XT[f][rows]; cs=np.cumsum(g[rows])
                    best=None
                    for p in range(1,m):
                        if fv[p]>np.float32(fv[p-1]+np.float32(1e-7)) and p>=msl and m-p>=msl:
                            sl=cs[p-1]; sr=tab['sg'][k]-sl; diff=(m-p)*sl-p*sr; sc=diff*diff/(p*(m-p))
                            if best is None or sc>best[0]: best=(sc,s+p)
                    if best is not None and (k not in cand or best[0]>cand[k][0]): cand[k]=(best[0],f,best[1])
            nxt=dict(start=[0]*(2*nk),cnt=[0]*(2*nk),node=[0]*(2*nk),flag=[0]*(2*nk),sg=[0.0]*(2*nk),spq=[0.0]*(2*nk))
            split={}; rank=0; nleft=[0]*nk
            for k in range(nk):
                s,m,node,flag=tab['start'][k],tab['cnt'][k],tab['node'][k],tab['flag'][k]
                if flag==1 and k in cand:
                    sc,f,bp=cand[k]; a=XT[f][order[f][bp-1]]; b=XT[f][order[f][bp]]
                    th=np.float64(a)/2.0+np.float64(b)/2.0
                    if th==np.float64(b): th=np.float64(a)
                    nl=bp-s; lc=n_nodes+2*rank; rank+=1
                    left[node]=lc; right[node]=lc+1; feat[node]=f; thr[node]=th; split[k]=(f,th); nleft[k]=nl
                    for j,(ss,cc,nn) in enumerate(((s,nl,lc),(s+nl,m-nl,lc+1))):
                        nxt['start'][2*k+j]=ss; nxt['cnt'][2*k+j]=cc; nxt['node'][2*k+j]=nn; nxt['flag'][2*k+j]=1
                else:
                    if flag==1:
                        left[node]=right[node]=-1; thr[node]=-2.0; den=tab['spq'][k]/m; val[node]=0.0 if abs(den)<1e-150 else (tab['sg'][k]/m)/den
                    nleft[k]=0 if flag==0 else m
                    nxt['start'][2*k]=s; nxt['cnt'][2*k]=m; nxt['node'][2*k]=node; nxt['flag'][2*k]=0 if flag==0 else 2
                    nxt['start'][2*k+1]=s+m
            n_nodes+=2*rank
            lbase=np.concatenate([[0],np.cumsum(nleft)[:-1]])
            newkey=key.copy()
            for i in range(n):
                k=key[i]; side=0
                if k in split: side=0 if np.float64(XT[split[k][0]][i])<=split[k][1] else 1
                newkey[i]=2*k+side
            neworder=np.full_like(order,-1)
            for f in range(d):
                lefts=0
                for p in range(n):
                    i=order[f][p]; nkv=newkey[i]; k=nkv>>1; isleft=not (nkv&1)
                    inseg=lefts-lbase[k]; s=tab['start'][k]
                    to = s+inseg if isleft else s+nleft[k]+(p-s-inseg)
                    assert neworder[f][to]==-1
                    neworder[f][to]=i
                    lefts+=isleft
            order=neworder; key=newkey; tab=nxt; level+=1
        nodeofkey=np.array(tab['node']); v=val[nodeofkey[key]]
        raw=raw+lr*v; stages.append(raw.copy())
        r=raw; loss=np.where(r<=-37,np.exp(r),np.where(r<=-2,np.log1p(np.exp(r)),np.where(r<=18,np.log(1+np.exp(r)),np.where(r<=33.3,r+np.exp(-r),r))))-y*r
        ts.append(2*loss.sum()/n); g=resid(y,raw)
        off=out['root'][-1]
        out['left'].append(np.where(left[:n_nodes]>=0,left[:n_nodes]+off,-1)); out['right'].append(np.where(right[:n_nodes]>=0,right[:n_nodes]+off,-1))
        out['feature'].append(feat[:n_nodes]); out['threshold'].append(thr[:n_nodes]); out['value'].append(val[:n_nodes]); out['n_node_samples'].append(nns[:n_nodes]); out['root'].append(off+n_nodes)
    trees={k:(np.concatenate(v) if k!='root' else np.array(v)) for k,v in out.items()}
    return trees,init,np.array(stages),np.array(ts)
