'use strict';
// The temporal upsampler following a moved chair through the drop-in: a full-size NativeRenderer runs only its
// G-buffer pass, a small one renders a frame per phase through SetPhaseOf, denoises it, and the full-size one
// integrates it with UpsampleTemporal; after `calls` calls both take UpdateWorld(world with the chair moved) and one
// more call follows.  With SetUpsampleFollow(true) before the first call the history survives the edit.
//
// argv: JSON {assetsDir, move: [x, y, z], width, height, scale, pipeline, calls, follow, out}
// stdout: JSON {masks: [hi, lo], uniform: [33 words of hi's last frame], keys: [...Object.keys(addon)]}; the
// full-size renderer's ReadUpsampleHistory() after the last call goes to `${out}.hist.f32`.
const fs = require('fs');
const { NativeRenderer, PASS, addon } = require('../../pathtracerdemo_amd/js/NativeRenderer');
const W = require('../../pathtracerdemo_amd/js/world');

async function main() {
  const req = JSON.parse(process.argv[2]);
  const rec = JSON.parse(fs.readFileSync(req.assetsDir + '/scene.json', 'utf8'));
  const worldOf = (move) => {
    const scene = W.sceneFromBackend(JSON.parse(JSON.stringify(rec)));
    if (move) scene.assets.find((a) => a.id === 'chair_instance_0').transform.position = move;
    W.ResourceManager.LoadCompiledAssets(req.assetsDir + '/meshes', W.sceneMeshNames(scene));
    const world = new W.World();
    world.LoadFromScene(scene);
    return world;
  };
  const make = (w, h) => new NativeRenderer(w, h, { pipeline: req.pipeline, device: 0, frameColor: true });
  const s = req.scale;
  const lo = make(req.width, req.height), hi = make(s * req.width, s * req.height);
  await lo.Initialize(worldOf(null));
  await hi.Initialize(worldOf(null));
  if (req.follow) hi.SetUpsampleFollow(true);
  const call = (k) => {
    const px = k % s, py = Math.floor(k / s) % s;
    hi.Update();
    hi.RunPass(PASS.GBUFFER);
    lo.SetPhaseOf(hi, s, px, py);
    lo.Render();
    lo.Denoise({ temporal: true, iterations: 2 });
    hi.UpsampleTemporal(lo, { px, py });
  };
  for (let k = 0; k < req.calls; ++k) call(k);
  const masks = [hi.UpdateWorld(worldOf(req.move)), lo.UpdateWorld(worldOf(req.move))];
  call(req.calls);
  fs.writeFileSync(`${req.out}.hist.f32`, Buffer.from(hi.ReadUpsampleHistory().buffer));
  const res = { masks, uniform: Array.from(hi.Uniform), keys: Object.keys(addon) };
  hi.Destroy();
  lo.Destroy();
  process.stdout.write(JSON.stringify(res));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
