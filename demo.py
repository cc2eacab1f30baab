"""demo.py -- same CLI as the reference's omnidata_tools/torch/demo.py:23-34:

    python demo.py --task {normal,depth} --img_path <file-or-dir> --output_path <dir>

It reads ./pretrained_models/omnidata_dpt_{normal,depth}_v2.ckpt (demo.py:36,62,80), writes
<stem>_<task>.png and <stem>_rgb.png (demo.py:127,134) and iterates glob(img_path+'/*') for a
directory (demo.py:158-160).  Extras for offline use: --weights PATH, --random-weights SEED,
--dtype (default 'mixed': within 1e-3 of the reference's fp32 forward; bf16 / fp16 / fp8 are faster throughput
modes that are not), --backbone unet (the version-1 UNet, demo.py:49-59: ./pretrained_models/omnidata_unet_normal_v1.pth;
fp16 unless --dtype bf16; --task depth needs --weights), --batch_size N (N > 1: a directory runs N images per forward through omnidata_amd.batch_infer,
same files, same pixels), --full_frame {squash,aspect} [--renormalize] (the whole image instead of the centre crop, <stem>_<task>.png at
the image's own size and <stem>_rgb.png = the image unchanged; any --batch_size; squash = a fixed 384x384 network input as
paper_code/oasis_eval_tta.py:324-339, aspect = the aspect-preserving size of modules/midas/transforms.py:94-160; --renormalize
makes the resized normals unit length again, oasis_eval_tta.py:339), --tta NAME [--tta_merger median|mean] (--task normal: test-time
augmentation, omnidata_amd/tta.py: the views of preset flip / whole / crops / oasis -- oasis_eval_tta.py:487-534, 40 views -- merged per pixel;
files as with --full_frame; --task depth --tta NAME --tta_align lstsq: the same for depth, every view fitted to a whole-image
anchor view by least squares before the merge, omnidata_amd/tta.py DepthTTA, DPT backbones only), --tiled [--tile_size 384
--tile_scale 1.0 --tile_overlap 0.25] (tiled high-resolution inference, omnidata_amd/tiled.py: overlapping tiles at the chosen pixel
scale, blended with feathered weights; depth tiles are aligned to a whole-image anchor; files as with --full_frame; excludes
--full_frame and --tta), --guided [--guided_radius 2 --guided_sigma_space 1.0 --guided_sigma_range 0.1] (with --full_frame: the map
goes to the image's own size through a joint bilateral filter guided by the image itself instead of the plain bilinear / bicubic
resize, so object boundaries land where the image has them; one forward per image, include/dptx.h "Guided upsampling").  The forward runs on an MI355X through libdptx.so; no CPU fallback.
"""
import argparse
import glob
import os
import sys
from pathlib import Path

import torch
from PIL import Image


def main(argv=None):
    parser = argparse.ArgumentParser(description="Visualize output for depth or surface normals")
    parser.add_argument("--task", dest="task", help="normal or depth")
    parser.set_defaults(task="NONE")
    parser.add_argument("--img_path", dest="img_path", help="path to rgb image")
    parser.add_argument("--output_path", dest="output_path", help="path to where output image should be stored")
    parser.add_argument("--weights", default=None, help="checkpoint path (default ./pretrained_models/omnidata_dpt_<task>_v2.ckpt)")
    parser.add_argument("--random-weights", type=int, default=None, metavar="SEED", help="seeded synthetic weights (offline)")
    parser.add_argument("--dtype", default="mixed", choices=["mixed", "fp16x3", "bf16x3", "fp16", "bf16", "fp8"],
                        help="mixed (default) matches the reference within 1e-3; bf16 / fp16 / fp8 are ~2x faster and do not")
    parser.add_argument("--backbone", default="vitb_rn50_384", choices=["vitb_rn50_384", "vitl16_384", "unet"],
                        help="vitb_rn50_384 = DPT-Hybrid (the v2 checkpoints); vitl16_384 = DPT-Large (demo.py:81, the v1 depth model); "
                             "unet = the version-1 UNet (demo.py:49-59)")
    parser.add_argument("--batch_size", type=int, default=1, metavar="N",
                        help="N > 1: a directory goes through the batched pipeline (omnidata_amd.batch_infer), N images per forward")
    parser.add_argument("--full_frame", default=None, choices=["squash", "aspect"],
                        help="keep the whole image (no centre crop) and write the map at the image's own size: squash = a fixed "
                             "square network input, aspect = the reference's aspect-preserving network size per image")
    parser.add_argument("--renormalize", action="store_true", help="--full_frame, normal: unit-length normals after the resize")
    parser.add_argument("--tta", default=None, choices=["flip", "whole", "crops", "oasis"],
                        help="--task normal: test-time augmentation with this view preset (omnidata_amd/tta.py), merged per pixel")
    parser.add_argument("--tta_merger", default="median", choices=["median", "mean"], help="--tta: how the views are merged")
    parser.add_argument("--tta_align", default=None, choices=["lstsq"],
                        help="--task depth --tta: fit every view to the whole-image anchor view (least-squares scale and shift) "
                             "before the merge; required for depth")
    parser.add_argument("--tiled", action="store_true",
                        help="tiled high-resolution inference (omnidata_amd/tiled.py): overlapping tiles, feathered blend, the map "
                             "at the image's own size; depth tiles are aligned to a whole-image anchor")
    parser.add_argument("--tile_size", type=int, default=384, help="--tiled: the network's short side for a tile")
    parser.add_argument("--tile_scale", type=float, default=1.0, help="--tiled: image pixels per network pixel along a tile's side")
    parser.add_argument("--tile_overlap", type=float, default=0.25, help="--tiled: the blend ramp as a fraction of the window, 0 .. 0.5")
    parser.add_argument("--guided", action="store_true",
                        help="--full_frame: guided upsampling to the image's own size (joint bilateral filter on the image) "
                             "instead of the bilinear / bicubic resize")
    parser.add_argument("--guided_radius", type=int, default=2, help="--guided: (2 * radius)^2 low-resolution taps per pixel, 1 .. 3")
    parser.add_argument("--guided_sigma_space", type=float, default=1.0, help="--guided: spatial sigma in low-resolution pixels")
    parser.add_argument("--guided_sigma_range", type=float, default=0.1, help="--guided: colour sigma in [0, 1] units")
    args = parser.parse_args(argv)

    if args.task not in ("normal", "depth"):
        print("task should be one of the following: normal, depth")
        sys.exit()
    if args.img_path is None or args.output_path is None:
        print("invalid file path!")
        sys.exit()
    if args.tta is not None and args.full_frame is not None:
        print("--tta excludes --full_frame")
        sys.exit()
    if args.tta is not None and args.task == "depth" and args.tta_align is None:
        print("--tta with --task depth needs --tta_align lstsq: the views of a depth map agree only up to a scale and a shift")
        sys.exit()
    if args.tta_align is not None and (args.tta is None or args.task != "depth"):
        print("--tta_align needs --task depth and --tta")
        sys.exit()
    if args.tiled and (args.tta is not None or args.full_frame is not None):
        print("--tiled excludes --full_frame and --tta")
        sys.exit()
    if args.tiled and not (0 <= args.tile_overlap <= 0.5 and args.tile_size >= 1 and args.tile_scale > 0):
        print("--tiled needs --tile_size >= 1, --tile_scale > 0 and --tile_overlap in [0, 0.5]")
        sys.exit()
    if args.guided and (args.full_frame is None or args.tta is not None or args.tiled):
        print("--guided needs --full_frame and excludes --tta and --tiled")
        sys.exit()
    if args.guided and not (1 <= args.guided_radius <= 3 and args.guided_sigma_space > 0 and args.guided_sigma_range > 0):
        print("--guided needs --guided_radius in 1 .. 3, --guided_sigma_space > 0 and --guided_sigma_range > 0")
        sys.exit()
    if args.backbone == "unet" and args.tiled and args.task == "depth":
        print("--backbone unet --task depth has no --tiled: the alignment is defined for the DPT depth models")
        sys.exit()
    if args.backbone == "unet" and args.tta is not None and args.task == "depth":
        print("--backbone unet --task depth has no --tta: the alignment is defined for the DPT depth models")
        sys.exit()

    from omnidata_amd.model import build_model
    from omnidata_amd import preprocess as pp

    os.makedirs(args.output_path, exist_ok=True)
    if not torch.cuda.is_available():
        raise RuntimeError("demo.py needs an AMD GPU: the DPT forward is implemented as HIP kernels only")
    device = torch.device("cuda:0")
    weights = args.weights
    if weights is None and args.random_weights is None:
        weights = "./pretrained_models/" + ("omnidata_dpt_normal_v2.ckpt" if args.task == "normal" else "omnidata_dpt_depth_v2.ckpt")
        if args.backbone == "vitl16_384" and args.task == "depth":
            weights = "./pretrained_models/omnidata_dpt_depth_v1.ckpt"  # the DPT-Large depth model (demo.py:80-81)
    unet = args.backbone == "unet"
    if args.renormalize and (args.full_frame is None or args.task != "normal"):
        print("--renormalize needs --full_frame and --task normal")
        sys.exit()
    if unet and args.full_frame == "aspect":
        print("--backbone unet takes --full_frame squash only: its network sizes are multiples of 64 up to 512, which the "
              "aspect-preserving size rule does not produce")
        sys.exit()
    if unet and args.full_frame is not None and args.task == "depth":
        print("--backbone unet --task depth has no batched pre-processing (rgb in [0, 1]): --full_frame is not available")
        sys.exit()
    if unet:
        # the version-1 model: rgb in [0, 1] (get_transform('rgb'), no normalisation) for both tasks, [B,out,H,W] results
        from omnidata_amd.unet import build_unet
        if args.weights is None and args.random_weights is None:
            if args.task == "depth":
                print("--backbone unet --task depth needs --weights (the reference publishes the v1 UNet for normals only)")
                sys.exit()
            weights = "./pretrained_models/omnidata_unet_normal_v1.pth"
        model = build_unet(args.task, weights=weights, random_weights=args.random_weights,
                           dtype="bf16" if args.dtype == "bf16" else "fp16", max_batch=min(max(args.batch_size, 1), 32))
        if args.task == "depth":
            args.batch_size = 1   # the batched pipeline's depth pre-processing normalises to [-1, 1]: per-image loop below
    else:
        model = build_model(args.task, weights=weights, random_weights=args.random_weights, dtype=args.dtype,
                            max_batch=max(args.batch_size, 1), backbone=args.backbone)
    model.to(device)
    if args.batch_size > 1 or args.full_frame is not None or args.tta is not None or args.tiled:
        from omnidata_amd.batch_infer import BatchPredictor
        p = Path(args.img_path)
        if not (p.is_file() or p.is_dir()):
            print("invalid file path!")
            sys.exit()
        files = [args.img_path] if p.is_file() else glob.glob(args.img_path + "/*")
        # the version-1 UNet takes sides that are multiples of 64 up to 512 (the model oasis_eval_tta.py evaluates)
        tta_options = dict(multiple=64, max_side=512) if unet and args.tta is not None else None
        tiled = None
        if args.tiled:
            tiled = dict(tile=args.tile_size, scale=args.tile_scale, overlap=args.tile_overlap)
            if unet:
                tiled.update(multiple=64, max_side=512)
        guided = None
        if args.guided:
            guided = dict(radius=args.guided_radius, sigma_space=args.guided_sigma_space, sigma_range=args.guided_sigma_range)
        BatchPredictor(model, args.task, batch_size=max(args.batch_size, 1), full_frame=args.full_frame,
                       renormalize=args.renormalize, tta=args.tta, tta_merger=args.tta_merger,
                       tta_options=tta_options, tta_align=args.tta_align, tiled=tiled, guided=guided).predict_to_dir(files, args.output_path, verbose=True)
        return

    def save_outputs(img_path, output_file_name):
        with torch.no_grad():
            save_path = os.path.join(args.output_path, f"{output_file_name}_{args.task}.png")
            print(f"Reading input {img_path} ...")
            img = Image.open(img_path)
            # Resize/CenterCrop/ToTensor(/Normalize) run on the GPU from the raw uint8 pixels (bit-identical to
            # the PIL/torchvision path of the reference; RGBA and other modes fall back to PIL inside)
            img_tensor = pp.image_to_input_gpu(img, "normal" if unet else args.task, device)
            pp.rgb_preview(img).save(os.path.join(args.output_path, f"{output_file_name}_rgb.png"))
            output = model(img_tensor).clamp(min=0, max=1)
            if unet and args.task == "depth":
                output = output.squeeze(1)   # [B,1,H,W] -> [B,H,W], what the DPT depth model returns
            if args.task == "depth":
                d512 = pp.depth_to_512_gpu(output)          # bicubic 384->512, clamp, 1-x on the GPU
                Image.fromarray(pp.colorize_viridis(d512.cpu().numpy())).save(save_path)
            else:
                Image.fromarray(pp.normal_to_u8_gpu(output[0]).cpu().numpy()).save(save_path)
            print(f"Writing output {save_path} ...")

    img_path = Path(args.img_path)
    if img_path.is_file():
        save_outputs(args.img_path, os.path.splitext(os.path.basename(args.img_path))[0])
    elif img_path.is_dir():
        for f in glob.glob(args.img_path + "/*"):
            save_outputs(f, os.path.splitext(os.path.basename(f))[0])
    else:
        print("invalid file path!")
        sys.exit()


if __name__ == "__main__":
    main()
