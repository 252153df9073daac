"""Large differential campaign (profiles/r01_parity_campaign.md): teacher-forced GPU vs oracle parity on all 100 PGDrive-v0 maps."""
import sys, time, json; sys.path.insert(0,'.')
import numpy as np, torch
from tests import util
from tests.test_parity_gpu import OBS_TOL, REW_TOL, _compare_rows, _flag_ties, _int_ties
from oracle import orc
from pgdrive_amd import _abi, bank
from pgdrive_amd.engine import Engine
descs = bank.load_descriptions()
out=[]
for mode, steps in (("driving", 1500), ("uniform", 600), ("straight", 900), ("driving-respawn", 500), ("idm-agent-respawn", 500)):
    n_envs=1024
    # (last streams, round 4: respawn-mode traffic -- every IDM vehicle drives from the first step: the dense rows of bench.py;
    # then the same with the ego driven by the IDM policy, IDM_agent)
    mb, sb = util.make_banks(descs, n_maps=100, **(dict(traffic_mode="respawn") if mode.endswith("respawn") else {}))
    cfg=_abi.make_config(n_envs, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=1, seed=11, idm_agent=1 if mode.startswith("idm-agent") else 0)
    eng=Engine(cfg,mb,sb); ora=orc.Oracle(cfg,mb,sb); ora.enable_margins()
    ids=np.arange(n_envs)%100
    o0=ora.reset(ids); g0=eng.reset(ids).cpu().numpy()
    assert np.abs(g0-o0).max()<OBS_TOL
    rng=np.random.default_rng(17)
    st=dict(steps=0,flag_mismatch=0,obs=0.0,rew=0.0,pose=0.0,beams=0,grazing=0,int_mismatch=0,done=0,active_traffic=0)
    t0=time.time(); worst={}
    ties=st.setdefault("ties", util.Ties("campaign "+mode))
    for t in range(steps):
        if mode.startswith("driving"): act=util.driving_actions(rng,n_envs)
        elif mode=="uniform": act=rng.uniform(-1,1,size=(n_envs,1,2)).astype(np.float32)
        else:
            act=np.zeros((n_envs,1,2),np.float32); act[...,1]=1.0; act[...,0]=rng.normal(0,0.05,size=(n_envs,1))
        oo,orw,od,ofl=ora.step(act,threads=64); mg=ora.margins()
        go,grw,gd,gfl=eng.step(torch.from_numpy(act).cuda()); eng.sync()
        go=go.cpu().numpy().astype(np.float64); grw=grw.cpu().numpy().astype(np.float64); gd=gd.cpu().numpy(); gfl=gfl.cpu().numpy().astype(np.uint32)
        same=(gfl==ofl)&(gd==od)
        # every mismatch is a tie only where the oracle's decision margins say so (tests/util.py: admissible); the rest is counted as
        # flag_mismatch / int_mismatch / beams_not_admitted or stays in "obs"
        st["steps"]+=same.size; flag_tie=_flag_ties(eng,st,same,mg); st["done"]+=int(od.sum())
        head=np.where(same[:,:,None],np.abs(go-oo),0.0)[:,0,:34]
        # a body whose nearest point sits on the 50 m broad-phase radius is a neighbour on one side only: the 16 neighbour
        # floats then differ wholesale (counted where the row's NEIGHBOUR margin confirms it)
        flip=(head[:,18:].max(axis=1)>OBS_TOL)&(head[:,:18].max(axis=1)<=OBS_TOL)&util.admissible("NEIGHBOUR",mg[util.MG["NEIGHBOUR"]][:,0])
        ties.add_slots("NEIGHBOUR",np.pad(flip[:,None],((0,0),(0,mg.shape[2]-1))),mg)
        st["neighbour_boundary_rows"]=st.get("neighbour_boundary_rows",0)+int(flip.sum())
        go_cmp=go.copy(); go_cmp[flip,0,18:34]=oo[flip,0,18:34]
        _compare_rows(eng,ora,st,go_cmp,oo,same,mg)  # sets obs / obs_state / beams / grazing
        st["rew"]=max(st["rew"],float(np.abs(grw-orw)[same].max()))
        f,i,ei=ora.get_state(); gf,gi,gei=eng.get_state()
        agree=(gi==i).all(axis=0)&(gei==ei).all(axis=0)[:,None]
        # (an env whose flags differ -- a contact seen on one side only -- was reset on one side: its integers are not compared twice)
        flag_env=(~same).any(axis=1)
        _int_ties(gi,i,gei,ei,mg,st,flag_tie)  # int_ties (verified, cascades of a verified flag tie included) / int_mismatch
        st["int_mismatch_in_flag_mismatch_envs"]=st.get("int_mismatch_in_flag_mismatch_envs",0)+int((~agree)[flag_env].sum())
        st["active_traffic"]+=int((i[0,:,1:]==2).sum())
        # IDM neighbour search: traffic spawns on a 10 m grid, so a leader exactly MAX_DIST = 30 m ahead is "found" or "not
        # found" by the last bit of the lane coordinate (also in the reference's fp64); such a vehicle gets a different
        # throttle on the two sides: counted, excluded from the pose statistic
        tie=util.idm_tie(gf,f,mg); ties.add_slots("LEADER",tie&agree,mg)
        st["idm_30m_ties"]=st.get("idm_30m_ties",0)+int((tie&agree).sum())
        for fld in ("X","Y","THETA","SPEED"):
            dd=np.abs(gf[_abi.SF[fld]].astype(np.float64)-f[_abi.SF[fld]])[agree&~tie]
            if fld=="THETA": dd=np.minimum(dd,np.abs(dd-2*np.pi))
            st["pose"]=max(st["pose"],float(dd.max()))
        util.compare_state(gf,f,agree&~tie,worst)  # all 26 float fields (tests/util.py STATE_TOL), in units of their tolerance
        f32=util.round_state_f32(f); ora.set_state(f32,i,ei); eng.set_state(f32,i,ei)
    st["state_fields_x_tol"]={k:round(v,3) for k,v in worst.items()}
    st["mode"]=mode; st["seconds"]=round(time.time()-t0,1)
    st["ties"]=dict(ties.summary(), cases=ties.cases, rejected=ties.rejected)  # admitted ties by class, with their margins
    print(json.dumps(st)); out.append(st); eng.close()
open('gpurun_out/campaign.json','w').write(json.dumps(out,indent=1))
