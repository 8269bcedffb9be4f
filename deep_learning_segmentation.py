#!/usr/bin/env python3
"""Label the Gaussians of a 3DGS PLY by majority vote over segmented camera views — MI355X build.

Drop-in for the reference script of the same name: same functions, same CLI flags
(--ply_file --camera_file --input_dir --output_dir --output_file --model), same PLY-in / PLY-out
contract.  The per-Gaussian projection + vote (reference lines 43-82, 252-308) runs in hand-written HIP
kernels behind libgsx.so; PLY parsing/writing is native too.  The 2-D segmentation networks stay what
they are in the reference (Hugging Face / Ultralytics models, imported lazily): they need weights that
are fetched by name, so `--segmap_dir` lets a run consume the `<image>_segmap.npy` files the reference
itself writes next to every segmented image (reference line 165) instead of running a network.  What follows the
network - arg-max and nearest resize of SegFormer's logits, the compositing of YOLO's instances (reference lines 85-124,
142-144), Mask2Former's post_process_instance_segmentation (156-158) - runs in HIP kernels too, and the class map goes from
the network to the vote without leaving the GPU.

Added flags: --segmap_dir DIR, --n_classes C (default: 150 for the ADE20K models, 80 for YOLO), --gpus N
(informational), --mask2former_map {segments,classes} (default segments: a Mask2Former map holds segment ids in acceptance
order, as the reference's does; classes: each segment's class id instead).
Several GPUs: `python -m torch.distributed.run --nproc-per-node N deep_learning_segmentation.py
...` — every rank segments and stages its contiguous block of the cameras, the packed class maps are all-gathered over
RCCL and every rank votes its slab of the Gaussians (3d_gaussian_splatting_project_amd/dist.py, protocol v4).
--smooth_k N [--smooth_rounds R] [--fill_unlabeled] (default off) cleans the finished labels with the majority filter over
the N nearest neighbours (3D_clustering/smooth_labels.py) before the file is written; --fill_unlabeled only fills the
Gaussians no view saw.
--split_k N [--split_max_dist D] [--split_min_size S] [--split_max_instances M] (default off) then turns the classes into
objects: the connected components of every label over the N nearest neighbours (3D_clustering/split_labels.py), -1 ignored;
the largest object gets id 0 and the instance table is printed.
--labeler {vote,lift} (default vote).  lift: instead of projecting each Gaussian's centre, every class map is lifted through
the rasterizer's own blend (Context.lift_view): a splat takes the class of the pixels it actually colours, weighted by its
blend weight T * alpha * G, so a splat behind a wall no longer takes the wall's class.  Needs the PLY's splat attributes
(scale_*, rot_*, opacity, f_dc_*); uses the VIEWER's camera convention, not the reference labeler's; single GPU.
--lift_min_weight W (default 0): splats whose summed weight over all views stays below W are labelled -1.
--associate [--assoc_min_overlap F] [--assoc_min_size N] [--assoc_max_instances M] (default off): the maps hold SEGMENT ids,
numbered per image (Mask2Former's default map), and every map first goes through Context.assoc_view, which renames its
segments to the global instances most of their Gaussians already carry (a segment matches when at least the fraction F of its
Gaussians, default 0.3, carry the instance; segments of fewer than N Gaussians are left out; at most M instances, default 255).
The relabelled map is voted or lifted with n_classes = M; the _segmap.npy side files stay the raw maps.  Single GPU: the
association is ordered over the views.
--label_maps_dir DIR and --reproject_iou (default off) go back from the finished labels - after --smooth_k - to the views:
the splats are uploaded again with their labels and every camera that had a class map is rendered as a label frame
(Context.label_view) at that map's own size, fx and fy scaled by map size / camera size as the lift scales them.
--label_maps_dir writes the frames as <img_name>_labelmap.npy (int32, -1 = no label); --reproject_iou accumulates the
contingency table of (rendered label map, input class map) over those views on the GPU and prints the IoU of every class
present: how well the 3-D labelling reproduces the maps it was made from.  Both need the PLY's splat attributes, work with
either labeler and run on one GPU.  The frames use the VIEWER's camera convention, as --labeler lift does, not the reference
labeler's: for voted labels the table therefore also measures that mismatch.  Neither goes with --associate or --split_k,
whose labels are not the maps' classes.
--depth_maps_dir DIR [--depth_quantile Q] (default off, Q = 0.5) renders the same views - every camera that had a class map, at
that map's size, fx and fy scaled likewise - as depth frames (Context.depth_view): <img_name>_depth.npy is the float32
view-space depth of the surface, the first fragment at which the accumulated alpha reaches Q (NaN = no surface), and
<img_name>_surface.npy the int32 PLY row of the splat that is that surface (-1 = none).  Needs the PLY's splat attributes, not
the labels; works with every other flag; one GPU; the VIEWER's camera convention.
"""
import argparse
import importlib
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
gsx = importlib.import_module("3d_gaussian_splatting_project_amd")
from importlib import import_module as _imp

_ply = _imp("3d_gaussian_splatting_project_amd.ply_io")

N_CLASSES = {"segformer": 150, "mask2former": 150, "yolo": 80}


def load_cameras(camera_file):
    """cameras.json -> list of camera dicts."""
    return gsx.load_cameras(camera_file)


def load_gaussians(ply_file):
    """Returns (gaussians, plydata): a structured array whose 'position' field is filled (scale and
    rotation stay zero, exactly like the reference) and the opened PLY for save_labeled_ply."""
    plydata = _ply.PlyData.read(ply_file)
    vertices = plydata["vertex"]
    gaussians = np.zeros(len(vertices), dtype=[("position", np.float32, 3), ("scale", np.float32, 3), ("rotation", np.float32, 4)])
    for axis, name in enumerate("xyz"):
        gaussians["position"][:, axis] = vertices.column_f32(name)
    return gaussians, plydata


def load_splat_attributes(plydata):
    """The attributes Context.upload_splats takes, from the PLY's vertex element: (xyz, scale, rot, opacity, f_dc); scale, rot
    and opacity are None where the file has none (the viewer's fallback)."""
    vertices = plydata["vertex"]
    names = set(vertices.properties)
    cols = lambda group: np.stack([vertices.column_f32(name) for name in group], axis=1)
    missing = [name for name in ("f_dc_0", "f_dc_1", "f_dc_2") if name not in names]
    if missing:
        raise ValueError(f"--labeler lift needs the splat attributes of the PLY: {', '.join(missing)} missing")
    full = all(name in names for name in ("scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "opacity"))
    return (cols("xyz"), cols(("scale_0", "scale_1", "scale_2")) if full else None,
            cols(("rot_0", "rot_1", "rot_2", "rot_3")) if full else None, vertices.column_f32("opacity") if full else None,
            cols(("f_dc_0", "f_dc_1", "f_dc_2")))


def project_gaussian(position, camera):
    """(x, y) pixel of a Gaussian centre in `camera`, or None — evaluated by the device kernel."""
    return gsx.project_gaussian(position, camera)


def initialize_model(model_type, device):
    """Load one of the reference's three segmentation networks (needs their weights to be available)."""
    if model_type == "segformer":
        from transformers import SegformerForSemanticSegmentation, SegformerImageProcessor
        name = "nvidia/segformer-b5-finetuned-ade-640-640"
        return SegformerImageProcessor.from_pretrained(name), SegformerForSemanticSegmentation.from_pretrained(name).to(device)
    if model_type == "mask2former":
        from transformers import AutoImageProcessor, Mask2FormerForUniversalSegmentation
        name = "facebook/mask2former-swin-large-ade-semantic"
        return AutoImageProcessor.from_pretrained(name), Mask2FormerForUniversalSegmentation.from_pretrained(name).to(device)
    if model_type == "yolo":
        from ultralytics import YOLO
        return None, YOLO("yolo11x-seg.pt")
    raise ValueError(f"Unknown model type: {model_type}")


def select_query_slots(class_queries_logits):
    """The selection of transformers' post_process_instance_segmentation, call for call, on the device the logits are on:
    class_queries_logits (Q, C + 1) -> (slot_query int64 (Q,), slot_score float32 (Q,), slot_label int64 (Q,)), the Q largest
    of the Q * C class probabilities in torch's own (unsorted) order.  The same query may fill several slots."""
    import torch
    num_queries, num_classes = class_queries_logits.shape[-2], class_queries_logits.shape[-1] - 1
    scores = torch.nn.functional.softmax(class_queries_logits, dim=-1)[:, :-1]
    scores_per_image, topk_indices = scores.flatten(0, 1).topk(num_queries, sorted=False)
    return torch.div(topk_indices, num_classes, rounding_mode="floor"), scores_per_image, topk_indices % num_classes


def _segment_image_device(image, processor, model, device, model_type, ctx, mask2former_map="segments", n_classes=None):
    """The device half of segment_image: network -> int32 (H, W) class map as a torch tensor on ctx's GPU, -1 = no class.
    The network's output never leaves the device: SegFormer logits, YOLO instances and Mask2Former queries go through libgsx's
    own kernels (Context.segmap_from_logits / segmap_from_masks / segmap_from_queries: torch.argmax's rule, OpenCV's nearest
    resize, the reference's instance loop, transformers' post_process_instance_segmentation - reference lines 85-124, 142-144,
    156-158).  mask2former_map: "segments" stores segment ids in acceptance order, as the reference does; "classes" stores each
    segment's class id.  n_classes: what the vote was begun with - a segment id must fit."""
    import torch
    width, height = image.size
    if model_type == "yolo":
        res = model(image, verbose=False)[0]
        orig_height, orig_width = res.orig_shape
        masks = getattr(res, "masks", None)
        if masks is None or res.boxes is None:
            return ctx.segmap_from_masks(None, None, None, (orig_width, orig_height))
        K = min(int(masks.data.shape[0]), int(res.boxes.cls.shape[0]))     # the reference zips the masks with the boxes
        return ctx.segmap_from_masks(masks.data[:K], res.boxes.cls[:K], res.boxes.conf[:K], (orig_width, orig_height))
    inputs = {k: v.to(device) for k, v in processor(images=image, return_tensors="pt").items()}
    with torch.no_grad():
        outputs = model(**inputs)
    if model_type == "segformer":
        return ctx.segmap_from_logits(outputs.logits[0], (width, height))
    if mask2former_map not in ("segments", "classes"):
        raise ValueError(f"Unknown Mask2Former map: {mask2former_map}")
    slot_query, slot_score, slot_label = select_query_slots(outputs.class_queries_logits[0])
    if mask2former_map == "segments" and n_classes is not None and int(slot_query.numel()) > n_classes:
        raise ValueError(f"{int(slot_query.numel())} queries may give as many segment ids: --n_classes must be at least that")
    return ctx.segmap_from_queries(outputs.masks_queries_logits[0], slot_query, slot_score, (width, height), slot_label=slot_label,
                                   labels=mask2former_map == "classes")


def _save_segmap(image_path, output_dir, seg_map):
    base = os.path.splitext(os.path.basename(image_path))[0]
    np.save(os.path.join(output_dir, f"{base}_segmap.npy"), seg_map)


def segment_image(image_path, output_dir, processor, model, device, model_type, ctx=None, mask2former_map="segments"):
    """int32 (H, W) class map of one image, -1 = no class; also saved as <image>_segmap.npy (reference line 165).
    The map is made on the GPU (_segment_image_device) and copied down here; assign_labels votes the device map instead and
    copies it down afterwards.  The reference's side-by-side PNG (its lines 198-214) is not written."""
    from PIL import Image
    os.makedirs(output_dir, exist_ok=True)
    image = Image.open(image_path)
    own = ctx is None
    ctx = ctx or gsx.Context()
    try:
        seg_map = _segment_image_device(image, processor, model, device, model_type, ctx, mask2former_map).cpu().numpy()
    finally:
        if own:
            ctx.close()
    _save_segmap(image_path, output_dir, seg_map)
    return seg_map


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def assign_labels(gaussians, cameras, input_dir, output_dir, model_type="mask2former", segmap_dir=None, n_classes=None,
                  ctx=None, mask2former_map="segments", labeler="vote", splats=None, lift_min_weight=0.0, associate=False,
                  assoc_min_overlap=0.3, assoc_min_size=1, assoc_max_instances=255):
    """Majority-vote label per Gaussian (int32, -1 = never visible), bit-identical to the reference.

    Cameras whose `<img_name>.png` is missing from input_dir are skipped with a warning, as in the
    reference; the remaining ones are voted in order (the order decides ties).

    labeler="lift": the maps are lifted through the rasterizer's blend instead (Context.lift_view, each at the map's own
    size with fx, fy scaled by map size / image size); splats = load_splat_attributes(plydata); a splat whose summed weight
    stays below lift_min_weight gets -1.

    associate: the maps hold per-image segment ids; each goes through Context.assoc_view first and its relabelled device map,
    a class map of assoc_max_instances instance ids, is what the labeler sees."""
    if labeler not in ("vote", "lift"):
        raise ValueError(f"Unknown labeler: {labeler}")
    lift = labeler == "lift"
    if lift and splats is None:
        raise ValueError("labeler='lift' needs the splat attributes (load_splat_attributes)")
    if model_type not in N_CLASSES:
        raise ValueError(f"Unknown model type: {model_type}")
    n_classes = n_classes or N_CLASSES[model_type]
    if associate:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("--associate runs on one GPU: the association is ordered over the views")
        n_segments, n_classes = 254, int(assoc_max_instances)   # what a raw map may hold; what the labeler is begun with
    todo = []
    for camera in cameras:
        img_path = os.path.join(input_dir, camera["img_name"] + ".png")
        if not os.path.exists(img_path):
            print(f"Warning: Image {camera['img_name']} not found")
            continue
        todo.append((camera, img_path))
    processor = model = device = None
    if segmap_dir is None and todo:
        import torch
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        processor, model = initialize_model(model_type, device)
    world, rank = _world()
    if lift and world > 1:
        raise ValueError("--labeler lift runs on one GPU")
    own = ctx is None
    ctx = ctx or gsx.Context()
    if own:
        gsx.bind_to_gpu_numa_node(ctx.device)   # maps, pinned staging and packer threads next to this rank's GPU
    try:
        # one process per GPU: this rank segments and stages its contiguous block of the processed cameras; the packed
        # maps are then all-gathered and every rank votes its slab of the Gaussians (dist.py, protocol v4).  A rank
        # may end up without any camera (more GPUs than images): it still takes part in every collective.
        lo, hi = gsx.dist.view_range(len(todo), rank, world) if world > 1 else (0, len(todo))
        total = max(1, len(todo))
        if lift:
            ctx.upload_splats(*splats)
            ctx.lift_begin(n_classes)
            view = lambda camera, seg_map, size: ctx.lift_view(camera, seg_map)   # fx, fy scaled by map size / camera size
        else:
            ctx.upload_positions(gaussians)
            ctx.vote_begin(n_classes, min(lo, total - 1), total)
            view = ctx.vote_view
        if associate:
            if lift:
                ctx.upload_positions(gaussians)
            ctx.assoc_begin(n_segments, n_classes, assoc_min_overlap, assoc_min_size)
            labeler_view = view
            view = lambda camera, seg_map, size: labeler_view(camera, ctx.assoc_view(camera, seg_map, size)[1], size)
        for camera, img_path in todo[lo:hi]:
            print(f"Processing image {os.path.basename(img_path)}...")
            if segmap_dir is not None:
                seg_map = np.load(os.path.join(segmap_dir, camera["img_name"] + "_segmap.npy"))
                view(camera, seg_map, _image_size(img_path))
                continue
            from PIL import Image
            os.makedirs(output_dir, exist_ok=True)
            image = Image.open(img_path)
            seg_dev = _segment_image_device(image, processor, model, device, model_type, ctx, mask2former_map,
                                            n_segments if associate else n_classes)
            view(camera, seg_dev, image.size)                   # the map goes from the network to the vote on the device ...
            _save_segmap(img_path, output_dir, seg_dev.cpu().numpy())   # ... and is copied down behind it, for the .npy only
        if associate:
            print(f"Association: {ctx.assoc_num_instances()} instances found, {ctx.assoc_num_dropped()} segments dropped")
        if world > 1:
            return gsx.dist.exchange_labels_gather(gsx.dist.GpuGatherShard(ctx), cap_views=total)
        return ctx.lift_finalize(lift_min_weight) if lift else ctx.vote_finalize()
    finally:
        if own:
            ctx.close()


def reproject_labels(splats, labels, cameras, input_dir, map_dir, n_classes, label_maps_dir=None, reproject_iou=False):
    """The finished labels as label frames of the cameras that had a class map (an image in input_dir; the map is
    <img_name>_segmap.npy in map_dir), each at its map's size: written to label_maps_dir as <img_name>_labelmap.npy and / or
    compared with the maps.  -> the contingency table int64 (n_classes + 1, n_classes + 1), row = rendered label + 1, column =
    map label + 1, summed over the views (zeros without reproject_iou).  Prints one IoU line per class present."""
    table = np.zeros((n_classes + 1, n_classes + 1), np.int64)
    if label_maps_dir is not None:
        os.makedirs(label_maps_dir, exist_ok=True)
    with gsx.Context() as ctx:
        ctx.upload_splats(*splats, labels=labels)
        for camera in cameras:
            if not os.path.exists(os.path.join(input_dir, camera["img_name"] + ".png")):
                continue
            seg_map = np.load(os.path.join(map_dir, camera["img_name"] + "_segmap.npy"))
            h, w = seg_map.shape
            frame = ctx.label_view(camera, w, h, n_classes, to_host=label_maps_dir is not None)
            if label_maps_dir is not None:
                np.save(os.path.join(label_maps_dir, camera["img_name"] + "_labelmap.npy"), frame)
            if reproject_iou:
                import torch
                seg_dev = torch.from_numpy(np.ascontiguousarray(seg_map)).to(torch.device("cuda", ctx.device))
                table += ctx.label_map_tables([ctx.label_map_device()], [seg_dev], n_classes, n_classes)[0]
    if reproject_iou:
        iou = gsx.iou_from_table(table)
        print("Reprojection IoU (rendered label map against input class map):")
        for b in range(n_classes + 1):
            rendered, given = int(table[b].sum()), int(table[:, b].sum())
            if rendered or given:
                print(f"Class {b - 1}: IoU {iou[b, b]:.6f} ({rendered} rendered, {given} input pixels)")
    return table


def write_depth_maps(splats, cameras, input_dir, map_dir, depth_maps_dir, quantile=0.5):
    """The depth frames (Context.depth_view) of the cameras that had a class map (an image in input_dir; the map is
    <img_name>_segmap.npy in map_dir), each at its map's size, fx and fy scaled to it: <img_name>_depth.npy, float32 view-space
    depth of the surface (the first fragment at which the accumulated alpha reaches `quantile`; NaN where there is none), and
    <img_name>_surface.npy, int32 row of that splat in the PLY (-1: none).  -> the names written."""
    os.makedirs(depth_maps_dir, exist_ok=True)
    written = []
    with gsx.Context() as ctx:
        ctx.upload_splats(*splats)
        for camera in cameras:
            if not os.path.exists(os.path.join(input_dir, camera["img_name"] + ".png")):
                continue
            h, w = np.load(os.path.join(map_dir, camera["img_name"] + "_segmap.npy"), mmap_mode="r").shape
            frame = ctx.depth_view(camera, w, h, quantile, surface_only=True)
            np.save(os.path.join(depth_maps_dir, camera["img_name"] + "_depth.npy"), frame.surface_z.astype(np.float32))
            np.save(os.path.join(depth_maps_dir, camera["img_name"] + "_surface.npy"), frame.surface_index)
            written.append(camera["img_name"])
    return written


def _shutdown(failed=False):
    """Leave a torch.distributed run.  After a failure on THIS rank the peers may be blocked in a collective this rank
    will never join: no barrier then, the process ends with a non-zero code and the launcher takes the others down."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        if dist.is_initialized():
            if failed:
                import sys
                import traceback
                traceback.print_exc()
                sys.stdout.flush()
                sys.stderr.flush()
                os._exit(1)
            dist.barrier()
            dist.destroy_process_group()


def _world():
    """(world size, rank) of a torch.distributed run (python -m torch.distributed.run ... this_script.py);
    initialises the process group on first use.  (1, 0) for a plain single-process run."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 1, 0
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("GSX_DIST_BACKEND", "nccl")      # "gloo": functional rehearsal on one GPU
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return dist.get_world_size(), dist.get_rank()


def save_labeled_ply(output_file, plydata, labels):
    """All original vertex properties + a trailing `int label`, binary little endian."""
    plydata.write(output_file, labels=np.asarray(labels, dtype=np.int32))


def make_parser():
    parser = argparse.ArgumentParser(description="Add labels to gaussians PLY file")
    parser.add_argument("--ply_file", help="Input PLY file with gaussians data")
    parser.add_argument("--camera_file", help="JSON file with camera data")
    parser.add_argument("--input_dir", help="Directory containing input images")
    parser.add_argument("--output_dir", help="Output directory to saved segmented input images")
    parser.add_argument("--output_file", help="Output PLY file with labels")
    parser.add_argument("--model", choices=["segformer", "mask2former", "yolo"], default="mask2former",
                        help="Choose segmentation model: mask2former or yolo")
    parser.add_argument("--segmap_dir", default=None, help="read <img_name>_segmap.npy from here instead of running a model")
    parser.add_argument("--mask2former_map", choices=["segments", "classes"], default="segments",
                        help="what a Mask2Former map stores: segment ids in acceptance order, as the reference does, or class ids")
    parser.add_argument("--n_classes", type=int, default=None, help="number of classes (labels -1..C-1)")
    parser.add_argument("--gpus", type=int, default=1, help="GPUs of this node (N>1: launch with torch.distributed.run)")
    parser.add_argument("--smooth_k", type=int, default=0, help="clean the labels with a majority filter over this many nearest "
                        "neighbours (0: off)")
    parser.add_argument("--smooth_rounds", type=int, default=1, help="rounds of that filter")
    parser.add_argument("--fill_unlabeled", action="store_true", help="the filter only fills Gaussians no view saw (label -1), "
                        "from their labelled neighbours")
    parser.add_argument("--split_k", type=int, default=0, help="split every label into its connected components over this many "
                        "nearest neighbours, largest first (0: off)")
    parser.add_argument("--split_max_dist", type=float, default=None, help="neighbours farther apart than this are not joined")
    parser.add_argument("--split_min_size", type=int, default=1, help="components of fewer Gaussians become -1")
    parser.add_argument("--split_max_instances", type=int, default=0, help="keep only this many of the largest components (0: all)")
    parser.add_argument("--labeler", choices=["vote", "lift"], default="vote", help="vote: the reference's majority vote over projected "
                        "centres; lift: class maps lifted through the rasterizer's blend (occlusion-aware, the viewer's camera convention)")
    parser.add_argument("--lift_min_weight", type=float, default=0.0, help="lift: splats whose summed blend weight stays below this "
                        "are labelled -1")
    parser.add_argument("--associate", action="store_true", help="the maps hold per-image segment ids: associate them across the "
                        "views through the Gaussians before they are voted or lifted (instance labels; single GPU)")
    parser.add_argument("--assoc_min_overlap", type=float, default=0.3, help="associate: a segment takes an instance that at least "
                        "this fraction of its Gaussians already carry")
    parser.add_argument("--assoc_min_size", type=int, default=1, help="associate: segments of fewer Gaussians are left out")
    parser.add_argument("--assoc_max_instances", type=int, default=255, help="associate: at most this many instances (<= 255)")
    parser.add_argument("--label_maps_dir", default=None, help="write the finished labels as label frames of the views, "
                        "<img_name>_labelmap.npy at each class map's size (needs the splat attributes; single GPU)")
    parser.add_argument("--reproject_iou", action="store_true", help="print the per-class IoU of those label frames against the "
                        "input class maps (the viewer's camera convention, as --labeler lift)")
    parser.add_argument("--depth_maps_dir", default=None, help="write the depth frames of the views: <img_name>_depth.npy (float32 "
                        "view-space depth of the surface) and <img_name>_surface.npy (int32 PLY row of the surface splat) at each "
                        "class map's size (needs the splat attributes; single GPU)")
    parser.add_argument("--depth_quantile", type=float, default=None, help="the surface is where the accumulated alpha reaches this "
                        "(0 < q <= 1, default 0.5)")
    return parser


def split_labels(gaussians, labels, k, max_dist=None, min_size=1, max_instances=0):
    """Classes into objects (Context.split_labels) over the finished labels, the unlabelled Gaussians (-1) left out; prints
    the instance table."""
    with gsx.Context() as ctx:
        labels, table = ctx.split_labels(gaussians["position"], labels, k=min(int(k), len(labels)), max_dist=max_dist, min_size=min_size,
                                         max_instances=max_instances, ignore_label=-1)
    print(f"{len(table['size'])} instances:")
    for m, (lab, size) in enumerate(zip(table["label"], table["size"])):
        print(f"Instance {m}: label {lab}, {size} gaussians")
    return labels


def smooth_labels(gaussians, labels, k, rounds=1, fill_unlabeled=False):
    """The k-nearest-neighbour majority filter (Context.smooth_labels) over the finished labels; fill_unlabeled: unlabelled
    neighbours cast no vote and only unlabelled Gaussians change."""
    with gsx.Context() as ctx:
        labels, changed = ctx.smooth_labels(gaussians["position"], labels, k=min(int(k), len(labels)), rounds=rounds,
                                            ignore_label=-1 if fill_unlabeled else None, fill_only=fill_unlabeled)
    for r, ch in enumerate(changed):
        print(f"Smoothing round {r + 1}: {ch} labels changed")
    return labels


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.fill_unlabeled and args.smooth_k <= 0:
        parser.error("--fill_unlabeled needs --smooth_k")
    if args.split_k <= 0 and (args.split_max_dist is not None or args.split_min_size != 1 or args.split_max_instances != 0):
        parser.error("--split_max_dist, --split_min_size and --split_max_instances need --split_k")
    if not args.associate and (args.assoc_min_overlap != 0.3 or args.assoc_min_size != 1 or args.assoc_max_instances != 255):
        parser.error("--assoc_min_overlap, --assoc_min_size and --assoc_max_instances need --associate")
    reproject = args.label_maps_dir is not None or args.reproject_iou
    if reproject and (args.associate or args.split_k > 0):
        raise ValueError("--label_maps_dir and --reproject_iou compare the labels with the maps' classes: not with --associate or --split_k")
    if reproject and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--label_maps_dir and --reproject_iou run on one GPU")
    if args.depth_quantile is not None and args.depth_maps_dir is None:
        parser.error("--depth_quantile needs --depth_maps_dir")
    quantile = 0.5 if args.depth_quantile is None else args.depth_quantile
    if not 0.0 < quantile <= 1.0:
        parser.error("--depth_quantile must be in (0, 1]")
    if args.depth_maps_dir is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--depth_maps_dir runs on one GPU")

    print("Loading cameras...")
    cameras = load_cameras(args.camera_file)
    print("Loading gaussians...")
    gaussians, plydata = load_gaussians(args.ply_file)
    splats = load_splat_attributes(plydata) if args.labeler == "lift" or reproject or args.depth_maps_dir is not None else None
    print("Assigning labels...")
    try:
        labels = assign_labels(gaussians, cameras, args.input_dir, args.output_dir, model_type=args.model,
                               segmap_dir=args.segmap_dir, n_classes=args.n_classes, mask2former_map=args.mask2former_map,
                               labeler=args.labeler, splats=splats if args.labeler == "lift" else None,
                               lift_min_weight=args.lift_min_weight, associate=args.associate,
                               assoc_min_overlap=args.assoc_min_overlap, assoc_min_size=args.assoc_min_size,
                               assoc_max_instances=args.assoc_max_instances)
    except BaseException:
        _shutdown(failed=True)
        raise
    _shutdown()
    if int(os.environ.get("RANK", "0")) != 0:
        return          # every rank holds the same labels; rank 0 writes the file
    if args.smooth_k > 0:
        print("Smoothing labels...")
        labels = smooth_labels(gaussians, labels, args.smooth_k, args.smooth_rounds, args.fill_unlabeled)
    if args.split_k > 0:
        print("Splitting labels into instances...")
        labels = split_labels(gaussians, labels, args.split_k, args.split_max_dist, args.split_min_size, args.split_max_instances)
    if reproject:
        print("Rendering label frames...")
        reproject_labels(splats, labels, cameras, args.input_dir, args.segmap_dir if args.segmap_dir is not None else args.output_dir,
                         args.n_classes or N_CLASSES[args.model], args.label_maps_dir, args.reproject_iou)
    if args.depth_maps_dir is not None:
        print("Rendering depth frames...")
        write_depth_maps(splats, cameras, args.input_dir, args.segmap_dir if args.segmap_dir is not None else args.output_dir,
                         args.depth_maps_dir, quantile)
    print("Saving labeled PLY file...")
    save_labeled_ply(args.output_file, plydata, labels)
    print(f"Done! Labeled PLY file saved as {args.output_file}")

    values, counts = np.unique(labels, return_counts=True)
    print("\nLabel statistics:")
    print(f"Total gaussians: {len(labels)}")
    print(f"Number of unique labels: {len(values)}")
    print("Label counts:")
    for value, count in zip(values, counts):
        print(f"Label {value}: {count} gaussians ({100 * count / len(labels):.2f}%)")


if __name__ == "__main__":
    main()
