"""Times the libsdhip VAE decoder and encoder at full SD-1.5 size (development tool)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sonicdiffusionbayeslab_amd.vae import HipVaeDecoder, HipVaeEncoder, VaeConfig, make_synthetic_vae_state_dict
cfg = VaeConfig(sample_size=64)
sd = make_synthetic_vae_state_dict(cfg)
dec = HipVaeDecoder(cfg, sd)
for b in (1, 8):
    lat = torch.randn(b, 4, 64, 64, device="cuda")
    for _ in range(2): out = dec.decode(lat, 1 / 0.18215)
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(3): out = dec.decode(lat, 1 / 0.18215)
    torch.cuda.synchronize(); dt = (time.time() - t0) / 3
    print(f"VAE decode batch {b}: {dt*1e3:.1f} ms  ({dt/b*1e3:.2f} ms/image, {2.514*b/dt:.0f} TFLOP/s)  finite={bool(torch.isfinite(out).all())}")
# encoder: 0.558 TMAC = 1.117 TFLOP per 512x512 image (3x3 convs 0.503, shortcut / attention projections 0.012, QK^T + PV
# of the 4096-token mid attention 0.017, entry conv 0.001 TMAC ... summed from the graph of AutoencoderKL.encode)
enc = HipVaeEncoder(cfg, sd)
for b in (1, 8):
    img = torch.rand(b, 3, 512, 512, device="cuda")
    for _ in range(2): out = enc.encode(img)
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(3): out = enc.encode(img)
    torch.cuda.synchronize(); dt = (time.time() - t0) / 3
    print(f"VAE encode batch {b}: {dt*1e3:.1f} ms  ({dt/b*1e3:.2f} ms/image, {1.117*b/dt:.0f} TFLOP/s)  finite={bool(torch.isfinite(out).all())}")
